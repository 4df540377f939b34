"""The edge-weighted run on the card (include/chanvese_hip.h, "Edge-weighted length") against the numpy restatement of the definition
(geodesic_util.py): per-iteration trace rows and final level sets of every case in FAST and STRICT arithmetic; weight one against
cvh_run on a twin context; the stop rule, determinism, split calls, what the context is after a call, refusals on live contexts.
Tolerance: 1e-9 relative on means and norms, 1e-9 max(1, max|u|) on the level set -- the bar of the four-phase kernels, compared as
test_gpu_multiphase.py compares."""
import ctypes as C

import numpy as np
import pytest

import geodesic_util as G
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


def make(capi, planes, u, gq, p, mode="fast"):
    h, w = u.shape
    ctx = capi.Context(h, w, len(planes), capi.make_params(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in p.items()}))
    ctx.set_option("math_mode", MODES[mode])
    ctx.set_image(planes)
    ctx.set_levelset(u)
    if gq is not None:
        ctx.set_edge_map(gq)
    return ctx


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_cases_match_the_restatement(capi, case, mode):
    h, w, ch, which, kind = case
    planes, u, gq = G.case_inputs(h, w, ch, kind)
    p = G.params_of(which)
    r, rsteps, rtrace = G.case_reference(case)
    ctx = make(capi, planes, u, None if kind == "sobel" else gq, p, mode)
    try:
        if kind == "sobel":
            ctx.edge_map_from(ctx, G.EDGE_K)                                  # the plane cvh_edge_map builds, not an uploaded one
        steps, norm, trace = capi.geodesic_run(ctx, G.ITERATIONS, trace=True)
        got = ctx.get_levelset()
        after = ctx.get_edge_map()
    finally:
        ctx.close()
    assert steps == rsteps == G.ITERATIONS and trace.shape == rtrace.shape
    rel = np.abs(trace - rtrace) / np.abs(rtrace)
    e = np.abs(got - r).max() / max(1.0, np.abs(r).max())
    print(G.case_id(case), mode, "trace", rel.max(axis=1), "u", e)
    assert np.isfinite(trace).all() and rel.max() <= 1e-9, rel
    assert norm == trace[-1, -1]
    assert e <= 1e-9
    assert np.array_equal(after, gq)                                          # the edge plane is unchanged by a run


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [(24, 64, 1), (67, 65, 3), (M.SEAM_H, 130, 1)], ids=lambda s: "x".join(map(str, s)))
def test_weight_one_is_cvh_run(capi, shape, mode):
    """gq = 32768 everywhere: the level set and the norm after 6 iterations are cvh_run's on a twin context, to the same bound -- a
    check that does not pass through the new restatement"""
    h, w, ch = shape
    planes, u, gq = G.case_inputs(h, w, ch, "ones")
    a, twin = make(capi, planes, u, gq, G.OTHER, mode), make(capi, planes, u, None, G.OTHER, mode)
    try:
        steps, norm, trace = capi.geodesic_run(a, G.ITERATIONS, trace=True)
        tsteps, tnorm = twin.run(G.ITERATIONS)
        x, y = a.get_levelset(), twin.get_levelset()
    finally:
        a.close()
        twin.close()
    e = np.abs(x - y).max() / max(1.0, np.abs(y).max())
    print(shape, mode, "u", e, "norm", abs(norm - tnorm) / tnorm)
    assert steps == tsteps == G.ITERATIONS
    assert e <= 1e-9 and abs(norm - tnorm) <= 1e-9 * tnorm


def stop_context(capi, mode="fast"):
    tol, k = G.stop_case()
    planes, u, gq = G.case_inputs(*G.STOP_SHAPE, "random")
    return make(capi, planes, u, gq, dict(G.DEFAULT, tol=tol), mode), k


@pytest.mark.parametrize("sync_every,before", [(None, 0), ("k", 0), (None, 1)], ids=["inside-a-chunk", "last-of-a-chunk", "even-count"])
def test_stop_rule(capi, sync_every, before):
    """the restatement stops at iteration k (odd, 2 < k < the chunk of 32): so does the card, with exactly k trace rows, and launches
    enqueued behind the stop change nothing -- the level set is that of a run with max_steps = k, bit for bit"""
    a, k = stop_context(capi)
    c, _ = stop_context(capi)
    try:
        stop = a.get_stop_condition()
        assert stop > 0
        if before:
            assert capi.geodesic_run(a, before)[0] == before and capi.geodesic_run(c, before)[0] == before
            k -= before
            assert k % 2 == 0 and k >= 2
        if sync_every:
            a.set_option("sync_every", k)
        steps, norm, trace = capi.geodesic_run(a, 10 * k, trace=True)
        ksteps, knorm, ktrace = capi.geodesic_run(c, k, trace=True)
        print("stop at", steps, "of", k, "norm", norm, "stop", stop)
        assert steps == k and ksteps == k and trace.shape == (k, 3)
        assert np.array_equal(bits(trace), bits(ktrace)) and norm == knorm
        assert norm <= stop and (k < 2 or trace[k - 2, -1] > stop)
        assert np.array_equal(bits(a.get_levelset()), bits(c.get_levelset()))
    finally:
        a.close()
        c.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_determinism_and_split_calls(capi, mode):
    planes, u, gq = G.case_inputs(67, 65, 3, "random")
    runs = []
    for split in ((6,), (6,), (2, 4)):
        ctx = make(capi, planes, u, gq, G.OTHER, mode)
        try:
            traces = [capi.geodesic_run(ctx, n, trace=True)[2] for n in split]
            runs.append((ctx.get_levelset(), np.vstack(traces)))
        finally:
            ctx.close()
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(bits(x), bits(y))                              # two runs: the same bits
    same = all(np.array_equal(bits(x), bits(y)) for x, y in zip(runs[0], runs[2]))
    print(mode, "6 against 2 + 4:", "bit for bit" if same else "NOT bit for bit", [float(np.abs(x - y).max()) for x, y in zip(runs[0], runs[2])])
    assert same


def test_after_the_call_the_context_holds_the_new_levelset(capi):
    """every existing call sees it, and a two-phase run continued afterwards is the run after cvh_set_levelset of the same doubles"""
    h, w, ch = 24, 64, 1
    planes, u, gq = G.case_inputs(h, w, ch, "random")
    a = make(capi, planes, u, gq, G.DEFAULT)
    fresh = capi.Context(h, w, ch, capi.make_params(tol=0.0))
    try:
        a.enqueue_steps(3)                                                    # (an odd count: the current buffer is the other one)
        a.sync()
        v = a.get_levelset()
        assert capi.geodesic_run(a, 5)[0] == 5
        r = G.run(planes, v, gq, G.DEFAULT, 5)[0]
        got = a.get_levelset()
        assert np.abs(got - r).max() <= 1e-9 * max(1.0, np.abs(r).max())
        assert a.sync()[0] == 0                                               # a new run has begun
        assert np.array_equal(a.get_mask(), G.mask(got))
        fresh.set_image(planes)
        fresh.set_levelset(got)
        a.enqueue_steps(3)
        fresh.enqueue_steps(3)
        assert a.sync()[:2] == fresh.sync()[:2]
        assert np.array_equal(bits(a.get_levelset()), bits(fresh.get_levelset()))
        assert np.array_equal(a.get_edge_map(), gq)
    finally:
        a.close()
        fresh.close()


DEMO_RUNS = [f"plain mu={mu:g}" for mu in G.DEMO_MUS] + [f"edge mu={mu:g} K={K:g}" for mu in G.DEMO_MUS[1:] for K in G.DEMO_KS]


@pytest.mark.parametrize("name", DEMO_RUNS)
def test_demonstration_masks_are_the_restatements(capi, name):
    """the demonstration of the README row on the card: every run's mask equals the restatement's on every pixel on which the restatement
    is itself determinate (geodesic_util.demo_runs, `firm`: taken from the restatement alone) -- EVERY pixel for the runs the
    demonstration is about, plain at every mu and weighted at the best mu; of the further weighted runs at mu = 20 and 100, mu = 100
    K = 45 has pixels that are not firm (its arm is dissolving when the run ends).  The restatement's runs are computed once and shared;
    the edge map is built on the card from the plane the card's own Perona-Malik smoothed."""
    runs, best = G.demo_runs()
    assert best == 5.0 and set(DEMO_RUNS) == set(runs)
    img, _, _ = G.demo_scene()
    u0, _ = G.demo_start(img)
    mu = float(name.split("mu=")[1].split()[0])
    ctx = make(capi, [img], u0, None, G.demo_params(mu))
    src = capi.Context(64, 64, 1, capi.make_params())
    try:
        if name.startswith("edge"):
            src.set_image([img])
            src.perona_malik(*G.DEMO_PM)
            assert np.array_equal(src.get_image()[0], G.demo_smoothed(img))
            ctx.edge_map_from(src, float(name.split("K=")[1]))
        else:
            ctx.set_edge_map(np.full((64, 64), G.ONE, dtype=np.uint16))
        assert capi.geodesic_run(ctx, G.demo_steps(mu))[0] == G.demo_steps(mu)
        got = ctx.get_mask()
    finally:
        ctx.close()
        src.close()
    want, firm = runs[name][0], runs[name][4]
    print(name, "pixels that differ", int((got != want).sum()), "of them firm", int(((got != want) & firm).sum()), "pixels not firm", int((~firm).sum()))
    if name.startswith("plain") or f"mu={best:g} " in name:
        assert firm.all()
    assert np.array_equal(got[firm], want[firm])


def test_an_empty_region_gives_nan_means(capi):
    """FAST arithmetic, u = -1e30 everywhere: the far-field series gives H_eps = 0 exactly, so sum H = 0 and c1 = 0 / 0 = NaN -- no
    guard, no error; the NaN reaches the level set and the norm, and the stop rule never fires on it"""
    h, w = 9, 70
    planes, _, gq = G.case_inputs(h, w, 1, "random")
    a = make(capi, planes, np.full((h, w), -1e30), gq, G.DEFAULT, "fast")
    try:
        steps, norm, trace = capi.geodesic_run(a, 3, trace=True)
        assert steps == 3 and np.isnan(norm) and np.isnan(trace[0, 0]) and np.isfinite(trace[0, 1])
        assert np.isnan(a.get_levelset()).all()
        a.set_levelset(G.case_inputs(h, w, 1, "random")[1])                   # the context stays usable
        assert np.isfinite(capi.geodesic_run(a, 1, trace=True)[2]).all()
    finally:
        a.close()


def test_refusals(capi):
    L = capi.lib()
    h, w = 8, 160   # ("state" = 32 exists from 144 columns, a multiple of 16)
    planes, u, gq = G.case_inputs(h, w, 1, "random")
    mk = lambda: capi.Context(h, w, 1, capi.make_params(tol=0.0))
    a, state32, no_image, no_levelset, no_edge = mk(), mk(), mk(), mk(), mk()
    everyone = [a, state32, no_image, no_levelset, no_edge]
    try:
        for c in (a, state32, no_levelset, no_edge):
            c.set_image(planes)
        for c in (a, state32, no_image, no_edge):
            c.set_levelset(u)
        for c in (a, state32, no_image, no_levelset):
            c.set_edge_map(gq)
        state32.set_option("state", 32)
        out = (C.c_double * 16)()
        err = lambda: L.cvh_last_error(None).decode()
        run = lambda x: L.cvh_geodesic_run(x._h, 2, None, None, None, 0, None)
        before = a.get_levelset()
        for x, code, text in ((state32, ERR_ARG, 'the context has "state" = 32'), (no_image, ERR_STATE, "the context has no image"),
                              (no_levelset, ERR_STATE, "the context has no level set"), (no_edge, ERR_STATE, "the context has no edge plane")):
            assert run(x) == code and err().startswith("cvh_geodesic_run: " + text), err()
            pair = (C.c_void_p * 2)(a._h.value, x._h.value)
            assert L.cvh_geodesic_run_batch(pair, 2, 2, None, None, None, 0, None) == code
            assert err().startswith("cvh_geodesic_run_batch: member 1: " + text), err()
        assert L.cvh_geodesic_run(a._h, 2, None, None, out, -1, None) == ERR_ARG and "a trace needs" in err()
        twice = (C.c_void_p * 2)(a._h.value, a._h.value)
        assert L.cvh_geodesic_run_batch(twice, 2, 2, None, None, None, 0, None) == ERR_ARG
        assert L.cvh_geodesic_run_batch(twice, 0, 2, None, None, None, 0, None) == ERR_ARG
        assert capi.geodesic_geometry(1 << 14, 1 << 14)[1:] == (0, 0)        # (h w >= 2^28: no test makes such a plane)
        assert np.array_equal(bits(a.get_levelset()), bits(before))          # nothing was touched, everybody is usable
        assert capi.geodesic_run(a, 2)[0] == 2
        assert capi.geodesic_run(a, 0) == (0, 0.0, None)
        no_edge.edge_map_from(a, 30.0)
        assert capi.geodesic_run(no_edge, 1)[0] == 1
    finally:
        for c in everyone:
            c.close()
