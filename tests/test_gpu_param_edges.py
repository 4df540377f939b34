"""Every CSV flavour at the parameter, level-set and image edges of tests/param_edges_util.py, against the oracle.

Flavours (each pinned through launch_info(), so that a case cannot silently run another kernel): the tile kernel (kernel 0) FAST and
STRICT, the 1-pixel wave kernel (kernel 2) FAST and STRICT, both with 1 and 3 channels, the 2-pixel wave kernel (kernel 3) with 1 and 3
channels, the resident kernel, the FP32-state mode and a member of a fused batch (run_batch).  Each flavour runs five cases: every start and every image, and
every parameter set of the covering design (so every eps, mu, nu, dt and lambda value meets every flavour).

Bars, the suite's: level set within 1e-9 of max|u| after 1, 3 and 10 iterations, every trace row rtol 1e-9, the same steps_done (the
library's default tol 1e-3 is on: the all-zero image has stop condition 0), the mask equal.  Two exceptions, both measured on the
oracle itself rather than assumed:
- plateau starts (rect, circle outline): flat regions have gradient 0/eta, which amplifies a 1-ulp difference ~1e6 per iteration
  (tests/test_golden.py, test_gpu_matches_csv_fixture): 1e-9 over iterations 1-3, 1e-6 at 10;
- a checkpoint is compared only while the oracle's own trajectory is well-conditioned there: a 1-ulp perturbation of u0 must move the
  oracle by less than 1/100 of the bar.  With mu = 2.5 (P1: dt mu = 7.5; P2 on const / zero / pixel images) the curvature term of
  near-flat regions amplifies a 1-ulp difference to 1e-8 .. 1 of max|u| within 3 iterations, so those cases compare iteration 1 (and
  whatever else stays conditioned); every case compares at least iteration 1.
The FP32-state mode has its own bar (tests/test_gpu_state32.py): its first iteration is the FP64 oracle's rounded to float."""
import numpy as np
import pytest

import param_edges_util as E

pytestmark = pytest.mark.gpu

STRICT, FAST = 1, 2
# flavour: (shape, channels, options, launch_info kernel prefix, math)
FLAVOURS = {
    "tile_fast": ((37, 150), 1, dict(kernel=0, math_mode=FAST), "csv_step_kernel<1, ", "fast"),
    "tile_strict": ((37, 150), 1, dict(kernel=0, math_mode=STRICT), "csv_step_kernel<1, ", "strict"),
    "wave1_fast": ((41, 136), 1, dict(kernel=2, math_mode=FAST, resident=0), "csv_wave_kernel<1, true, ", "fast"),
    "wave1_strict": ((41, 136), 1, dict(kernel=2, math_mode=STRICT), "csv_wave_kernel<1, false, ", "strict"),
    "wave2_c1": ((40, 160), 1, dict(kernel=3, math_mode=FAST, resident=0), "csv_wave2_kernel<1, true, 3, ", "fast"),
    "wave2_c3": ((33, 144), 3, dict(kernel=3, math_mode=FAST), "csv_wave2_kernel<3, true, 3, ", "fast"),
    "resident": ((48, 160), 1, dict(resident=1), "csv_resident_kernel<", "fast"),
    "state32": ((40, 144), 1, dict(state=32, resident=0), "csv_wave2_kernel<1, true, 3, ", "fast"),
    # three channels in the 1-pixel wave kernel (every STRICT colour image, FAST below 0.6 Mpixel) and in the tile kernel
    "wave1_c3_fast": ((41, 136), 3, dict(kernel=2, math_mode=FAST), "csv_wave_kernel<3, true, ", "fast"),
    "wave1_c3_strict": ((41, 136), 3, dict(kernel=2, math_mode=STRICT), "csv_wave_kernel<3, false, ", "strict"),
    "tile_c3_fast": ((37, 150), 3, dict(kernel=0, math_mode=FAST), "csv_step_kernel<3, ", "fast"),
    "tile_c3_strict": ((37, 150), 3, dict(kernel=0, math_mode=STRICT), "csv_step_kernel<3, ", "strict"),
}
# A flavour's index chooses its images and seeds (case_inputs, tests/lopsided_util.py): pinned, so that a flavour added later leaves every
# earlier case its inputs.  0-7: the first eight of the table; 8: the member of a fused batch; from 9: in the order added.
INDEX = {f: i for i, f in enumerate(["tile_fast", "tile_strict", "wave1_fast", "wave1_strict", "wave2_c1", "wave2_c3", "resident", "state32",
                                     "batch", "wave1_c3_fast", "wave1_c3_strict", "tile_c3_fast", "tile_c3_strict"])}
assert set(INDEX) == set(FLAVOURS) | {"batch"}
CASES = [(f, k) for f in sorted(INDEX, key=INDEX.get) for k in range(5)]
CHECKPOINTS = (1, 3, 10)


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def case_inputs(oracle, flavour, k, shape, channels):
    fi = INDEX[flavour]
    pname = list(E.PARAMS)[k % 4]
    st, im = E.STARTS[k], E.IMAGES[(k + fi) % 5]
    h, w = shape
    pk = E.params(pname, channels, tol=1e-3)
    return pname, st, im, pk, E.start(oracle, st, h, w, pk["eps"], seed=k), E.image(im, h, w, channels, seed=fi)


def conditioned(oracle, planes, u0, pk, checkpoints=None):
    """max |du| / max |u| of the oracle at each checkpoint (CHECKPOINTS when not given) after a 1-ulp perturbation of u0 (about a third of
    the pixels up, a third down)."""
    rng = np.random.default_rng(5)
    up = u0 * (1 + rng.choice([-1.0, 0.0, 1.0], size=u0.shape) * 2.0 ** -52)
    p = oracle.make_params(**pk)
    out = {}
    for s in checkpoints if checkpoints is not None else CHECKPOINTS:
        a, da, _, _ = oracle.csv_run(planes, u0, p, s)
        b, db, _, _ = oracle.csv_run(planes, up, p, s)
        out[s] = np.inf if da != db else float(np.abs(a - b).max() / max(np.abs(a).max(), 1e-300))
    return out


def bar_for(st, s):
    return 1e-6 if (st in E.PLATEAU and s == 10) else 1e-9


def oracle_run(oracle, planes, u0, pk, s, float_state=False):
    """(u, steps_done, trace) of the oracle after at most s iterations; float_state: with its level set rounded to float after every
    iteration (tests/test_gpu_state32.py)."""
    p = oracle.make_params(**pk)
    if float_state:
        f32 = lambda a: a.astype(np.float32).astype(np.float64)
        u_c, done_c, tr_c = f32(u0), 0, []
        for _ in range(s):
            nrm, c1, c2 = oracle.csv_step(planes, u_c, p)
            u_c = f32(u_c)
            done_c += 1
            tr_c.append(list(c1) + list(c2) + [nrm])
            if nrm <= oracle.stop_condition(planes, pk["tol"]):
                break
        tr_c = np.array(tr_c)
    else:
        u_c, done_c, _, tr_c = oracle.csv_run(planes, u0, p, s)
    return u_c, done_c, tr_c


def check(oracle, what, planes, u0, pk, s, got, float_state=False):
    u_g, done_g, tr_g, m_g = got
    u_c, done_c, tr_c = oracle_run(oracle, planes, u0, pk, s, float_state)
    assert done_g == done_c, (what, done_g, done_c)
    scale = np.abs(u_c).max()
    err = float(np.abs(u_g - u_c).max() / scale)
    if float_state:
        # the float roundings that fell the other way, amplified by the recurrence (tests/test_gpu_state32.py: 2e-5 over 8 iterations)
        assert err <= (1e-9 if s == 1 else 2e-5), (what, err)
        assert (m_g != oracle.mask(u_c)).mean() <= 1e-4, what
        assert np.allclose(tr_g[:1], tr_c[:1], rtol=1e-9, atol=0), (what, tr_g[:1], tr_c[:1])
        return err
    assert err <= bar_for(what[2], s), (what, err)
    assert tr_g.shape == tr_c.shape and np.allclose(tr_g, tr_c, rtol=1e-9, atol=0), (what, np.abs(tr_g - tr_c).max())
    assert np.array_equal(m_g, oracle.mask(u_c)), (what, int((m_g != oracle.mask(u_c)).sum()))
    return err


def run_single(capi, flavour, planes, u0, pk, s):
    shape, channels, opts, prefix, math = FLAVOURS[flavour]
    h, w = shape
    with capi.Context(h, w, channels, capi.make_params(**pk)) as ctx:
        for key, v in opts.items():
            ctx.set_option(key, v)
        ctx.set_option("trace", s)
        ctx.set_image(planes)
        ctx.set_levelset(u0 if flavour != "state32" else u0.astype(np.float32).astype(np.float64))
        info = ctx.launch_info()
        assert info["kernel"].startswith(prefix) and info.get("math", math) == math, (flavour, info)
        if flavour == "state32":
            assert info["kernel"].endswith("true>"), info
        done, _ = ctx.run(s)
        return ctx.get_levelset(), done, ctx.get_trace(done), ctx.get_mask()


@pytest.mark.parametrize("flavour,k", CASES)
def test_flavour_at_parameter_edges(capi, oracle, flavour, k):
    if flavour == "batch":
        return _batch_case(capi, oracle, k)
    shape, channels = FLAVOURS[flavour][:2]
    pname, st, im, pk, u0, planes = case_inputs(oracle, flavour, k, shape, channels)
    if flavour == "state32":
        u0 = u0.astype(np.float32).astype(np.float64)
    cond = conditioned(oracle, planes, u0, pk)
    compared = []
    for s in CHECKPOINTS:
        what = (flavour, pname, st, im, s)
        if s > 1 and cond[s] > bar_for(st, s) / 100:
            continue
        check(oracle, what, planes, u0, pk, s, run_single(capi, flavour, planes, u0, pk, s), float_state=flavour == "state32")
        compared.append(s)
    assert compared and compared[0] == 1, (flavour, k, cond)


def _batch_case(capi, oracle, k):
    """Two members with different parameter sets, images and starts in one run_batch; each against the oracle with its own inputs."""
    h, w = 40, 160
    pname, st, im, pk, u0, planes = case_inputs(oracle, "batch", k, (h, w), 1)
    other = (k + 2) % 5
    pname2, st2, im2, pk2, u02, planes2 = case_inputs(oracle, "batch", other, (h, w), 1)
    cond = conditioned(oracle, planes, u0, pk)
    cond2 = conditioned(oracle, planes2, u02, pk2)
    compared = []
    for s in CHECKPOINTS:
        todo = [(i, c) for i, c in enumerate((cond, cond2)) if s == 1 or c[s] <= bar_for((st, st2)[i], s) / 100]
        if not todo:
            continue
        ctxs = []
        try:
            for p_, img_, u_ in ((pk, planes, u0), (pk2, planes2, u02)):
                c = capi.Context(h, w, 1, capi.make_params(**p_))
                ctxs.append(c)
                c.set_option("trace", s)
                c.set_image(img_)
                c.set_levelset(u_)
                # a member's own flow (what it would run alone); in the batch every member runs the fused kernel
                assert c.launch_info()["kernel"].startswith(("csv_wave", "csv_resident")), c.launch_info()
            out = capi.run_batch(ctxs, s)
            for i, c in enumerate(ctxs):
                if (i, (cond, cond2)[i]) not in todo:
                    continue
                args = ((pname, st, im), (pname2, st2, im2))[i]
                inputs = ((planes, u0, pk), (planes2, u02, pk2))[i]
                what = ("batch",) + args + (s,)
                done = out[i][0]
                check(oracle, what, inputs[0], inputs[1], inputs[2], s, (c.get_levelset(), done, c.get_trace(done), c.get_mask()))
                compared.append((i, s))
        finally:
            for c in ctxs:
                c.close()
    assert (0, 1) in compared and (1, 1) in compared, (k, cond, cond2)
