"""The convex relaxation on the card (include/chanvese_hip.h, "Convex relaxation") against the numpy restatement of the definition
(convex_util.py): every shape of multiphase_util.CASES x parameter sets A and B x STRICT and FAST x with and without a random edge
plane.  STRICT with means_every = 0 is bit-defined -- the means come from exact integer sums -- and is compared with ==; everything
else to 1e-9 absolute on v, qx, qy (all of order 1) and 1e-9 relative on the trace, the bar of the march flows.  Then determinism,
resumed calls, what the context is after a call, the disk scene's exact fixed point, and the refusals on live contexts."""
import ctypes as C

import numpy as np
import pytest

import convex_util as X

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


def same(a, b):
    """== on every element, a NaN equal to a NaN (the contract lets a NaN through, its payload is nobody's)"""
    return np.array_equal(a, b, equal_nan=True)


def worst(got, want, relative=False):
    """the largest |got - want| (relative: over |want|) where want is finite; -1 where the NaNs do not coincide"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return -1.0
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    e = np.abs(got[ok] - want[ok])
    if relative:
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(e == 0, 0.0, e / np.abs(want[ok]))
    return float(e.max())


def make(capi, planes, u, gq, p, mode="strict"):
    h, w = planes[0].shape
    ctx = capi.Context(h, w, len(planes), capi.make_params(mu=p["mu"], nu=p["nu"], lambda1=list(p["lambda1"]), lambda2=list(p["lambda2"])))
    ctx.set_option("math_mode", MODES[mode])
    ctx.set_image(planes)
    if u is not None:
        ctx.set_levelset(u)
    if gq is not None:
        ctx.set_edge_map(gq)
    return ctx


def cp(capi, p, **over):
    q = dict(tau=p["tau"], sigma=p["sigma"], stop_rms=-1.0, means_every=p["means_every"])
    q.update(over)
    return capi.make_convex_params(**q)


@pytest.mark.parametrize("edge", [0, 1], ids=["plain", "edge"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", list(X.SETS))
@pytest.mark.parametrize("shape", X.SHAPES, ids=X.shape_id)
def test_cases_match_the_restatement(capi, shape, which, mode, edge):
    planes, u, gq = X.case_inputs(*shape)
    p = X.SETS[which]
    ctx = make(capi, planes, u, gq, p, mode)
    try:
        steps, norm, trace = capi.convex_run(ctx, X.ITERATIONS, cp(capi, p, use_edge=edge), trace=True)
        v, qx, qy = ctx.relaxed(duals=True)
        level = ctx.get_levelset()
        rv, rqx, rqy, rsteps, rtrace = X.reference(shape, which, edge)
        assert steps == rsteps == X.ITERATIONS and trace.shape == rtrace.shape
        e = [worst(a, b) for a, b in ((v, rv), (qx, rqx), (qy, rqy))]
        et = worst(trace, rtrace, relative=True)
        print(X.shape_id(shape), which, mode, "edge" if edge else "plain", "v qx qy", e, "trace", et)
        assert 0 <= max(e) <= 1e-9 and min(e) >= 0 and 0 <= et <= 1e-9
        assert same(norm, trace[-1, -1])
        assert same(level, v - 0.5)                                           # the level set afterwards, one rounding per pixel
        assert np.array_equal(ctx.get_mask(), X.mask(v - 0.5))
        if mode == "strict":                                                  # means_every = 0: every input of every pixel is bit-defined
            ctx.set_levelset(u)
            assert capi.convex_run(ctx, X.ITERATIONS, cp(capi, p, use_edge=edge, means_every=0))[0] == X.ITERATIONS
            got = ctx.relaxed(duals=True)
            want = X.reference(shape, which, edge, 0)[:3]
            diff = [int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum()) for a, b in zip(got, want)]
            print("  means_every = 0: pixels that differ in v, qx, qy", diff)
            assert diff == [0, 0, 0]
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", list(X.SETS))
@pytest.mark.parametrize("shape", [(67, 65, 3), (X.M.SEAM_H, 130, 1)], ids=X.shape_id)
def test_determinism_and_resumed_calls(capi, shape, which, mode):
    """two runs give the same bits; 6 iterations in one call are 2 and then 4 resumed, bit for bit, trace included"""
    planes, u, gq = X.case_inputs(*shape)
    p = X.SETS[which]
    runs = []
    for split in ((6,), (6,), (2, 4)):
        ctx = make(capi, planes, u, gq, p, mode)
        try:
            traces = [capi.convex_run(ctx, n, cp(capi, p, use_edge=1, resume=k > 0), trace=True)[2] for k, n in enumerate(split)]
            runs.append(ctx.relaxed(duals=True) + (ctx.get_levelset(), np.vstack(traces)))
        finally:
            ctx.close()
    for x, y in zip(runs[0], runs[1]):
        assert np.array_equal(bits(x), bits(y))
    split_same = [bool(np.array_equal(bits(x), bits(y))) for x, y in zip(runs[0], runs[2])]
    print(X.shape_id(shape), which, mode, "6 against 2 + 4 (v, qx, qy, u, trace):", split_same)
    assert all(split_same)


def test_resume_does_not_read_the_levelset(capi):
    planes, u, gq = X.case_inputs(24, 64, 1)
    p = X.SET_A
    a, b = make(capi, planes, u, None, p), make(capi, planes, u, None, p)
    try:
        for c in (a, b):
            assert capi.convex_run(c, 3, cp(capi, p))[0] == 3
        b.set_levelset(-u)
        for c in (a, b):
            assert capi.convex_run(c, 3, cp(capi, p, resume=1))[0] == 3
        assert np.array_equal(bits(a.relaxed()), bits(b.relaxed())) and np.array_equal(bits(a.get_levelset()), bits(b.get_levelset()))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_weight_one_is_no_edge_plane(capi, mode):
    """use_edge = 1 with gq = 32768 everywhere is use_edge = 0, bit for bit"""
    planes, u, _ = X.case_inputs(67, 65, 3)
    p = X.SET_B
    a, b = make(capi, planes, u, np.full(u.shape, X.ONE, dtype=np.uint16), p, mode), make(capi, planes, u, None, p, mode)
    try:
        ra = capi.convex_run(a, X.ITERATIONS, cp(capi, p, use_edge=1), trace=True)
        rb = capi.convex_run(b, X.ITERATIONS, cp(capi, p, use_edge=0), trace=True)
        assert ra[:2] == rb[:2] and np.array_equal(bits(ra[2]), bits(rb[2]))
        for x, y in zip(a.relaxed(duals=True), b.relaxed(duals=True)):
            assert np.array_equal(bits(x), bits(y))
    finally:
        a.close()
        b.close()


def test_after_the_call_the_context_holds_the_thresholded_levelset(capi):
    """every existing call sees u = v - 0.5, and a two-phase run continued afterwards is the run after cvh_set_levelset of the same doubles"""
    h, w, ch = 24, 64, 1
    planes, u, gq = X.case_inputs(h, w, ch)
    p = X.SET_A
    a = make(capi, planes, u, gq, p, "fast")
    fresh = capi.Context(h, w, ch, capi.make_params(mu=p["mu"], nu=p["nu"], lambda1=list(p["lambda1"]), lambda2=list(p["lambda2"]), tol=0.0))
    try:
        a.enqueue_steps(3)                                                    # (an odd count: the current buffer is the other one)
        a.sync()
        start = a.get_levelset()
        assert capi.convex_run(a, 5, cp(capi, p, use_edge=1))[0] == 5
        st, _, _ = X.run(planes, start, gq, p, 5)
        got = a.get_levelset()
        assert np.array_equal(bits(got), bits(a.relaxed() - 0.5))
        assert np.abs(got - (st["v"] - 0.5)).max() <= 1e-9
        assert a.sync()[0] == 0                                               # a new run has begun
        assert np.array_equal(a.get_mask(), X.mask(got))
        fresh.set_option("math_mode", MODES["fast"])
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


@pytest.mark.parametrize("mode", list(MODES))
def test_the_disk_reaches_its_fixed_point(capi, mode):
    """the noisy disk at 64 x 64, lambda = 1e-3, stop_rms = 0: STRICT stops where the restatement stops, FAST within one iteration
    of it; the mask is the restatement's on every pixel in both modes"""
    img, _ = X.disk_scene()
    rv, rsteps, rtrace = X.disk_reference()
    ctx = make(capi, [img], X.M.starts(64, 64)[0], None, X.DISK, mode)
    try:
        steps, norm, trace = capi.convex_run(ctx, 64, cp(capi, X.DISK, stop_rms=0.0), trace=True)
        got = ctx.get_mask()
        v = ctx.relaxed()
    finally:
        ctx.close()
    print(mode, "steps", steps, "restatement", rsteps, "norms", trace[:, -1])
    assert norm == 0.0 and trace.shape[0] == steps
    assert steps == rsteps if mode == "strict" else abs(steps - rsteps) <= 1
    assert np.array_equal(got, X.mask(rv - 0.5)) and set(np.unique(v)) == {0.0, 1.0}


def test_max_steps_zero_and_the_members_own_stop(capi):
    planes, u, _ = X.case_inputs(24, 64, 1)
    ctx = make(capi, planes, u, None, X.SET_A)
    try:
        assert capi.convex_run(ctx, 0, cp(capi, X.SET_A)) == (0, 0.0, None)
        assert np.array_equal(ctx.relaxed(), X.mask(u).astype(np.float64)) and np.array_equal(ctx.get_levelset(), X.mask(u) - 0.5)
        steps, norm, trace = capi.convex_run(ctx, 40, cp(capi, X.SET_A, stop_rms=1e30), trace=True)   # stops after its first iteration
        assert steps == 1 and trace.shape == (1, 3) and norm == trace[0, 2]
    finally:
        ctx.close()


def test_refusals(capi):
    L = capi.lib()
    h, w = 8, 160   # ("state" = 32 exists from 144 columns, a multiple of 16)
    planes, u, gq = X.case_inputs(8, 4096, 1)
    planes, u, gq = [np.ascontiguousarray(planes[0][:, :w])], np.ascontiguousarray(u[:, :w]), np.ascontiguousarray(gq[:, :w])
    mk = lambda: capi.Context(h, w, 1, capi.make_params(tol=0.0, lambda1=[1e-4] * 3, lambda2=[1e-4] * 3))
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
        good = dict(tau=0.25, sigma=0.5, stop_rms=0.0, means_every=1, use_edge=1)
        par = lambda **over: capi.make_convex_params(**dict(good, **over))
        run = lambda x, q: L.cvh_convex_run(x._h, 2, C.byref(q), None, None, None, 0, None)
        assert capi.convex_run(a, 2, par())[0] == 2                           # a holds a relaxation state and a level set
        before = [a.get_levelset()] + list(a.relaxed(duals=True))
        for x, code, text in ((state32, ERR_ARG, 'the context has "state" = 32'), (no_image, ERR_STATE, "the context has no image"),
                              (no_levelset, ERR_STATE, "the context has no level set"), (no_edge, ERR_STATE, "the context has no edge plane")):
            assert run(x, par()) == code and err().startswith("cvh_convex_run: " + text), err()
            pair = (C.c_void_p * 2)(a._h.value, x._h.value)
            two = (type(par()) * 2)(par(), par())
            assert L.cvh_convex_run_batch(pair, 2, 2, two, None, None, None, 0, None) == code
            assert err().startswith("cvh_convex_run_batch: member 1: " + text), err()
        nan, inf = float("nan"), float("inf")
        for over, text in ((dict(tau=0.0), "tau must be"), (dict(tau=-1.0), "tau must be"), (dict(tau=nan), "tau must be"), (dict(tau=inf), "tau must be"),
                           (dict(sigma=0.0), "sigma must be"), (dict(sigma=nan), "sigma must be"), (dict(sigma=inf), "sigma must be"),
                           (dict(tau=0.5, sigma=0.2500001), "8 tau sigma"), (dict(stop_rms=nan), "stop_rms is NaN"), (dict(means_every=-1), "means_every")):
            assert run(a, par(**over)) == ERR_ARG and text in err(), (over, err())
        assert L.cvh_convex_run(a._h, 2, None, None, None, None, 0, None) == ERR_ARG
        assert run(no_edge, par(use_edge=0, resume=1)) == ERR_STATE and "no relaxation state" in err()
        assert L.cvh_get_relaxed(no_edge._h, None, None, None) == ERR_STATE
        assert L.cvh_convex_run(a._h, 2, C.byref(par()), None, None, out, -1, None) == ERR_ARG and "a trace needs" in err()
        twice = (C.c_void_p * 2)(a._h.value, a._h.value)
        two = (type(par()) * 2)(par(), par())
        assert L.cvh_convex_run_batch(twice, 2, 2, two, None, None, None, 0, None) == ERR_ARG
        assert L.cvh_convex_run_batch(twice, 0, 2, two, None, None, None, 0, None) == ERR_ARG
        assert capi.convex_geometry(1 << 14, 1 << 14)[1:] == (0, 0)          # (h w >= 2^28: no test makes such a plane)
        assert capi.convex_geometry(h, w) == capi.geodesic_geometry(h, w)
        after = [a.get_levelset()] + list(a.relaxed(duals=True))
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before, after))   # nothing was touched, everybody is usable
        assert capi.convex_run(a, 2, par(resume=1))[0] == 2
        assert capi.convex_run(no_edge, 1, par(use_edge=0))[0] == 1
        assert run(state32, par()) == ERR_ARG
    finally:
        for c in everyone:
            c.close()
