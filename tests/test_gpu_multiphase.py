"""The four-phase calls on the card (include/chanvese_hip.h, "Four phases") against the numpy restatement of the definition
(multiphase_util.py): per-iteration trace rows, final level sets and labels of every case in FAST and STRICT arithmetic; the stop rule,
determinism, what the contexts are after a call, refusals on live contexts, and that the read-only calls only read.
Tolerance: 1e-9 relative on means and norms, 1e-9 max(1, max|phi|) on the level sets -- the library's own bar between its flows, two
decades above what test_multiphase_restatement.py shows two summation orders to differ by on these very cases."""
import ctypes as C

import numpy as np
import pytest

import multiphase_util as M

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_STATE = 0, 1, 3
MODES = {"fast": 2, "strict": 1}


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def make_pair(capi, planes, u1, u2, pa, pb, mode="fast", planes_b=None):
    h, w = u1.shape
    out = []
    for p, u, pl in ((pa, u1, planes), (pb, u2, planes_b if planes_b is not None else planes)):
        ctx = capi.Context(h, w, len(planes), capi.make_params(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in p.items()}))
        ctx.set_option("math_mode", MODES[mode])
        ctx.set_image(pl)
        ctx.set_levelset(u)
        out.append(ctx)
    return out


def close(*ctxs):
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_cases_match_the_restatement(capi, case, mode):
    h, w, ch, which = case
    planes, u1, u2 = M.case_inputs(h, w, ch)
    pa, pb = M.params_of(which)
    r1, r2, rsteps, rtrace = M.case_reference(case)
    # B's planes are not read by the step: it holds another image (its stop condition, tol = 0 here, would be taken from it)
    a, b = make_pair(capi, planes, u1, u2, pa, pb, mode, planes_b=[255 - p for p in planes])
    try:
        first = capi.multiphase_means(a, b)
        steps, norms, trace = capi.multiphase_run(a, b, M.ITERATIONS, trace=True)
        g1, g2 = a.get_levelset(), b.get_levelset()
        lab = a.multiphase_labels_with(b)
        after = capi.multiphase_means(a, b)
    finally:
        close(a, b)
    assert steps == rsteps == M.ITERATIONS and trace.shape == rtrace.shape
    rel = np.abs(trace - rtrace) / np.abs(rtrace)
    scale = max(1.0, np.abs(r1).max(), np.abs(r2).max())
    e1, e2 = np.abs(g1 - r1).max() / scale, np.abs(g2 - r2).max() / scale
    keep = ~M.near_zero(r1, r2)
    print(M.case_id(case), mode, "trace", rel.max(axis=1), "phi1", e1, "phi2", e2, "labels left out", 1 - keep.mean())
    assert np.isfinite(trace).all() and rel.max() <= 1e-9, rel
    assert norms == (trace[-1, -2], trace[-1, -1])
    assert e1 <= 1e-9 and e2 <= 1e-9
    assert np.array_equal(first.ravel(), trace[0, :-2])                      # the means of the start are the first iteration's
    want = M.means(planes, r1, r2, pa["eps"])
    assert np.all(np.abs(after - want) <= 1e-9 * np.abs(want))
    assert 1 - keep.mean() <= 1e-3
    assert lab.dtype == np.uint8 and lab.max() <= 3
    assert np.array_equal(lab[keep], M.labels(r1, r2)[keep])
    assert np.array_equal(lab, M.labels(g1, g2))                              # and exactly the labels of the card's own level sets


def stop_pair(capi, mode="fast", **kw):
    tol, k = M.stop_case()
    planes, u1, u2 = M.case_inputs(*M.STOP_SHAPE)
    p = dict(M.DEFAULT, tol=tol, **kw)
    return make_pair(capi, planes, u1, u2, p, p, mode), k


@pytest.mark.parametrize("sync_every,before", [(None, 0), ("k", 0), (None, 1)], ids=["inside-a-chunk", "last-of-a-chunk", "even-count"])
def test_stop_rule(capi, sync_every, before):
    """the restatement stops at iteration k (2 < k < the chunk of 32): so does the card, with exactly k trace rows, and launches enqueued
    behind the stop change nothing -- the level sets are those of a run with max_steps = k, bit for bit.  k is odd: the stopping call ends
    with its one copy of each level set; with `before` = 1 iteration done by an earlier call it counts k - 1, even, and ends without"""
    (a, b), k = stop_pair(capi)
    (c, d), _ = stop_pair(capi)
    try:
        assert a.get_stop_condition() > 0
        if before:
            assert capi.multiphase_run(a, b, before)[0] == before and capi.multiphase_run(c, d, before)[0] == before
            k -= before
            assert k % 2 == 0 and k > 2
        if sync_every:
            a.set_option("sync_every", k)
        steps, norms, trace = capi.multiphase_run(a, b, 10 * k, trace=True)
        ksteps, knorms, ktrace = capi.multiphase_run(c, d, k, trace=True)
        print("stop at", steps, "of", k, "norms", norms, "stop", a.get_stop_condition(), b.get_stop_condition())
        assert steps == k and ksteps == k and trace.shape == (k, 6)
        assert np.array_equal(bits(trace), bits(ktrace)) and norms == knorms
        assert norms[0] <= a.get_stop_condition() and norms[1] <= b.get_stop_condition()
        assert max(trace[k - 2, -2] / a.get_stop_condition(), trace[k - 2, -1] / b.get_stop_condition()) > 1
        for x, y in ((a, c), (b, d)):
            assert np.array_equal(bits(x.get_levelset()), bits(y.get_levelset()))
    finally:
        close(a, b, c, d)


@pytest.mark.parametrize("mode", list(MODES))
def test_determinism_and_split_calls(capi, mode):
    case = (67, 65, 3, "other")
    planes, u1, u2 = M.case_inputs(67, 65, 3)
    pa, pb = M.params_of("other")
    runs = []
    for split in ((6,), (6,), (2, 4)):
        a, b = make_pair(capi, planes, u1, u2, pa, pb, mode)
        try:
            traces = [capi.multiphase_run(a, b, n, trace=True)[2] for n in split]
            runs.append((a.get_levelset(), b.get_levelset(), np.vstack(traces)))
        finally:
            close(a, b)
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(bits(x), bits(y))                              # two runs of the same pair: the same bits
    scale = max(1.0, np.abs(runs[0][0]).max(), np.abs(runs[0][1]).max())
    same = all(np.array_equal(bits(x), bits(y)) for x, y in zip(runs[0], runs[2]))
    print(mode, "6 against 2 + 4: bit for bit" if same else "6 against 2 + 4: not bit for bit",
          [float(np.abs(x - y).max()) for x, y in zip(runs[0], runs[2])])
    assert same   # (the header's own claim: the second call's initial sums are the first call's last sums, in both arithmetic modes)
    assert np.abs(runs[0][0] - runs[2][0]).max() <= 1e-9 * scale and np.abs(runs[0][1] - runs[2][1]).max() <= 1e-9 * scale
    assert np.all(np.abs(runs[0][2] - runs[2][2]) <= 1e-9 * np.abs(runs[0][2]))
    assert runs[0][2].shape == M.case_reference(case)[3].shape


def test_after_the_call_the_contexts_hold_the_new_levelsets(capi):
    """every existing call sees them, and a one-context run continued afterwards is the run after cvh_set_levelset of the same doubles"""
    h, w, ch = 24, 64, 1
    planes, u1, u2 = M.case_inputs(h, w, ch)
    a, b = make_pair(capi, planes, u1, u2, M.DEFAULT, M.DEFAULT)
    fresh = [capi.Context(h, w, ch, capi.make_params(tol=0.0)) for _ in range(2)]
    try:
        a.enqueue_steps(3)                                                    # (an odd count: A's current buffer is its other one)
        a.sync()
        v1 = a.get_levelset()
        b.run(2)
        v2 = b.get_levelset()
        assert capi.multiphase_run(a, b, 5)[0] == 5
        ref = M.run(planes, v1, v2, M.DEFAULT, M.DEFAULT, 5)
        for ctx, f, r in ((a, fresh[0], ref[0]), (b, fresh[1], ref[1])):
            u = ctx.get_levelset()
            assert np.abs(u - r).max() <= 1e-9 * max(1.0, np.abs(r).max())
            assert ctx.sync()[0] == 0                                         # a new run has begun
            assert np.array_equal(ctx.get_mask(), ((u.astype(np.float32)) > 0).astype(np.uint8))
            f.set_image(planes)
            f.set_levelset(u)
            assert ctx.components(cap=0)[0] == f.components(cap=0)[0]
            la, lb = ctx.contours(), f.contours()
            assert len(la) == len(lb) and all(np.array_equal(x, y) for x, y in zip(la, lb))
            ctx.enqueue_steps(3)
            f.enqueue_steps(3)
            assert ctx.sync()[:2] == f.sync()[:2]
            assert np.array_equal(bits(ctx.get_levelset()), bits(f.get_levelset()))
    finally:
        close(a, b, *fresh)


def test_read_only_calls_only_read(capi):
    h, w, ch = 24, 64, 1
    planes, u1, u2 = M.case_inputs(h, w, ch)
    a, b = make_pair(capi, planes, u1, u2, M.DEFAULT, M.DEFAULT)
    c, d = make_pair(capi, planes, u1, u2, M.DEFAULT, M.DEFAULT)
    try:
        from test_gpu_device_io import Hip   # (device buffers without torch: hipMalloc / hipMemcpy of the runtime in the process)
        hip = Hip()
        for x in (a, b, c, d):
            x.run(2)
        m1 = capi.multiphase_means(a, b)
        lab = a.multiphase_labels_with(b)
        d_lab = hip.upload(np.full((h, w), 9, dtype=np.uint8), offset=3)      # (a caller's buffer at an odd address)
        a.multiphase_labels_with(b, ptr=d_lab)                                # ordered behind, and in front of, the default stream
        assert np.array_equal(hip.get(d_lab, (h, w), np.uint8), lab)
        hip.free_all()
        assert np.array_equal(lab, a.get_mask() + 2 * b.get_mask())
        assert np.array_equal(m1, capi.multiphase_means(a, b))
        for x, y in ((a, c), (b, d)):
            assert x.run(3) == y.run(3)
            assert np.array_equal(bits(x.get_levelset()), bits(y.get_levelset()))
    finally:
        close(a, b, c, d)


def test_refusals(capi):
    L = capi.lib()
    h, w = 8, 160   # ("state" = 32 exists from 144 columns, a multiple of 16)
    planes, u1, u2 = M.case_inputs(h, w, 1)
    planes3 = M.case_inputs(h, w, 3)[0]
    mk = lambda hh=h, ww=w, ch=1, **kw: capi.Context(hh, ww, ch, capi.make_params(tol=0.0, **kw))
    a, b, other_shape, three, other_eps, state32, no_image, no_levelset = mk(), mk(), mk(h, w + 1), mk(ch=3), mk(eps=1.5), mk(), mk(), mk()
    everyone = [a, b, other_shape, three, other_eps, state32, no_image, no_levelset]
    try:
        for c in (a, b, other_eps, state32, no_levelset):
            c.set_image(planes)
        three.set_image(planes3)
        other_shape.set_image(M.case_inputs(h, w + 1, 1)[0])
        for c in (a, b, three, other_eps, state32, no_image):
            c.set_levelset(u1)
        other_shape.init_checkerboard()
        b.set_levelset(u2)
        state32.set_option("state", 32)
        out = (C.c_double * 16)()
        lab = np.zeros((h, w), dtype=np.uint8)
        labp = lab.ctypes.data_as(C.POINTER(C.c_uint8))
        err = lambda: L.cvh_last_error(None).decode()
        calls = {
            "cvh_multiphase_run": lambda x, y: L.cvh_multiphase_run(x, y, 2, None, None, None, 0, None),
            "cvh_multiphase_means": lambda x, y: L.cvh_multiphase_means(x, y, out),
            "cvh_multiphase_labels": lambda x, y: L.cvh_multiphase_labels(x, y, labp),
            "cvh_multiphase_labels_device": lambda x, y: L.cvh_multiphase_labels_device(x, y, None, None),
        }
        before = (a.get_levelset(), b.get_levelset())
        for name, call in calls.items():
            reads_image = name in ("cvh_multiphase_run", "cvh_multiphase_means")
            cases = [
                (None, b, ERR_ARG, "context a is NULL"), (a, None, ERR_ARG, "context b is NULL"), (a, a, ERR_ARG, "a and b are the same context"),
                (a, other_shape, ERR_ARG, f"a is {h} x {w}, b {h} x {w + 1}"), (three, a, ERR_ARG, "a has 3 channel(s), b 1"),
                (a, other_eps, ERR_ARG, "eps must be equal"), (state32, b, ERR_ARG, 'context a has "state" = 32'),
                (a, state32, ERR_ARG, 'context b has "state" = 32'), (a, no_levelset, ERR_STATE, "context b has no level set"),
                (no_levelset, b, ERR_STATE, "context a has no level set"),
            ]
            if reads_image:
                cases += [(a, no_image, ERR_STATE, "context b has no image"), (no_image, b, ERR_STATE, "context a has no image")]
            for x, y, code, text in cases:
                assert call(x._h if x else None, y._h if y else None) == code, (name, text, err())
                assert err().startswith(name + ": " + text), (name, text, err())
        assert L.cvh_multiphase_means(a._h, b._h, None) == ERR_ARG and "c is NULL" in err()
        assert L.cvh_multiphase_labels(a._h, b._h, None) == ERR_ARG and "labels is NULL" in err()
        assert L.cvh_multiphase_labels_device(a._h, b._h, labp, None) == ERR_ARG and "not device-accessible" in err()   # host memory
        assert L.cvh_multiphase_run(a._h, b._h, 2, None, None, out, -1, None) == ERR_ARG and "a trace needs" in err()
        if capi.device_count() >= 2:
            far = capi.Context(h, w, 1, capi.make_params(tol=0.0), device=1)
            everyone.append(far)
            far.set_image(planes)
            far.set_levelset(u2)
            assert calls["cvh_multiphase_run"](a._h, far._h) == ERR_ARG and "a is on device 0, b on device 1" in err()
        # NOT covered on the card: the h*w >= 2^28 refusal of the four calls (a plane of 2^28 doubles is 2 GiB per buffer, four buffers a
        # pair: no test makes one; cvh_multiphase_geometry's zeros for that shape stand in), and the different-devices refusal where the
        # machine has one device (the branch above)
        big = capi.multiphase_geometry(1 << 14, 1 << 14)
        assert big[1:] == (0, 0) and capi.multiphase_geometry(9, 130) == (61, 8, 6)
        # nothing was touched, everybody is usable
        assert np.array_equal(bits(a.get_levelset()), bits(before[0])) and np.array_equal(bits(b.get_levelset()), bits(before[1]))
        assert capi.multiphase_run(a, b, 2)[0] == 2
        no_levelset.set_levelset(u2)
        no_image.set_image(planes)
        assert capi.multiphase_run(no_image, no_levelset, 1)[0] == 1
    finally:
        close(*everyone)


def test_an_empty_region_gives_nan_means(capi):
    """the header's rule: a region whose weight sum is exactly 0 has the means 0 / 0 = NaN, as IEEE division gives -- no guard --, the NaN
    reaches both level sets and both norms with the next iteration, the stop rule never fires on it, and none of that is an error.
    FAST arithmetic, phi1 = -1e30 everywhere: the far-field series gives H_eps = 0 exactly, so w11 and w10 vanish."""
    h, w = 9, 70
    planes, _, u2 = M.case_inputs(h, w, 1)
    a, b = make_pair(capi, planes, np.full((h, w), -1e30), u2, M.DEFAULT, M.DEFAULT, "fast")
    try:
        c = capi.multiphase_means(a, b)
        assert np.isnan(c[0, 0]) and np.isnan(c[1, 0]) and np.isfinite(c[2:, 0]).all(), c
        import np_restatement as R
        h2, f = R.heaviside(u2), planes[0].astype(np.float64)                  # with H1 = 0: w01 = H2, w00 = 1 - H2
        want = np.array([(f * h2).sum() / h2.sum(), (f * (1 - h2)).sum() / (1 - h2).sum()])
        assert np.all(np.abs(c[2:, 0] - want) <= 1e-9 * np.abs(want))
        steps, norms, trace = capi.multiphase_run(a, b, 3, trace=True)
        assert steps == 3 and np.isnan(norms).all() and np.isnan(trace[0, :2]).all()
        assert np.isnan(a.get_levelset()).all() and np.isnan(b.get_levelset()).all()
        a.set_levelset(u2)                                                    # the contexts stay usable
        b.set_levelset(np.roll(u2, 1, axis=1))
        assert np.isfinite(capi.multiphase_means(a, b)).all()
    finally:
        close(a, b)
