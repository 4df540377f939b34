"""The localised-regions calls on the card (include/chanvese_hip.h, "Localised regions") against the numpy restatement of the
definition (localized_util.py): final level set and trace of every case in FAST and STRICT arithmetic, the integer sums and the means
held to ==, the bit-level properties, the stop rule, what the context is after a call, every refusal, and the demonstration.
Tolerance: localized_util.tolerance() on u -- ten times what perturbing H_eps by 2 ulp per pixel does to the restatement over the
cases' six iterations -- and trace_tolerance(h, w) on ||d||."""
import ctypes as C

import numpy as np
import pytest

import localized_util as L

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


def make(capi, planes, u, p, mode="fast"):
    h, w = u.shape
    ctx = capi.Context(h, w, len(planes), capi.make_params(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in p.items()}))
    ctx.set_option("math_mode", MODES[mode])
    ctx.set_image(planes)
    ctx.set_levelset(u)
    return ctx


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", L.CASES, ids=L.case_id)
def test_cases_match_the_restatement(capi, case, mode):
    h, w, ch, rad, which = case
    planes, u = L.case_inputs(h, w, ch)
    ref, rsteps, rtrace = L.case_reference(case)
    ctx = make(capi, planes, u, L.params_of(which), mode)
    try:
        steps, norm, trace = capi.localized_run(ctx, rad, L.ITERATIONS, trace=True)
        got = ctx.get_levelset()
    finally:
        ctx.close()
    tol, ttol = L.tolerance(), L.trace_tolerance(h, w)
    err, terr = np.abs(got - ref).max(), np.abs(trace - rtrace).max()
    print(L.case_id(case), mode, "max|du|", err, "of", tol, "max|d norm|", terr, "of", ttol)
    assert tol <= 1e-7
    assert steps == rsteps == L.ITERATIONS and trace.shape == rtrace.shape
    assert np.isfinite(got).all() and err <= tol
    assert terr <= ttol and norm == trace[-1]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", [(67, 65, 3, 6, "other"), (3, L.SEGMENT + 1, 1, 4, "default"), (9, 300, 1, 127, "default"), (2, 2, 1, 127, "other")],
                         ids=L.case_id)
def test_means_are_the_quotients_of_exact_sums(capi, case, mode):
    h, w, ch, rad, which = case
    planes, u = L.case_inputs(h, w, ch)
    ctx = make(capi, planes, u, L.params_of(which), mode)
    try:
        m = ctx.localized_means(rad)
        only = ctx.localized_means(rad, want=("a",))
    finally:
        ctx.close()
    wq = m["wq"]
    c1, c2, A, S = L.means_of(planes, wq, rad)
    assert np.array_equal(m["a"], A) and np.array_equal(only["a"], A) and list(only) == ["a"]
    for k in range(ch):
        assert np.array_equal(m["s"][k], S[k])
        assert np.array_equal(bits(m["c1"][k]), bits(c1[k])) and np.array_equal(bits(m["c2"][k]), bits(c2[k]))
    off = np.abs(wq.astype(np.int64) - L.weights(u).astype(np.int64)).max()
    print(L.case_id(case), mode, "max |wq - restatement's|", off)
    assert off <= 2


@pytest.mark.parametrize("mode", list(MODES))
def test_weights_at_zero_and_far_from_the_front(capi, mode):
    h, w, rad = 9, 70, 2
    planes, _ = L.case_inputs(h, w, 1)
    u = np.zeros((h, w))
    u[:, :20], u[:, 50:] = 1e300, -1e300
    ctx = make(capi, planes, u, L.DEFAULT, mode)
    try:
        m = ctx.localized_means(rad)
    finally:
        ctx.close()
    wq = m["wq"]
    assert np.all(wq[:, 20:50] == L.ONE // 2) and np.all(wq[:, :20] == L.ONE) and np.all(wq[:, 50:] == 0)
    B = L.window_counts(h, w, rad) * np.uint64(L.ONE) - m["a"]
    assert np.array_equal(np.isnan(m["c1"][0]), m["a"] == 0) and np.array_equal(np.isnan(m["c2"][0]), B == 0)
    assert (m["a"] == 0).any() and (B == 0).any()
    assert np.array_equal(m["a"], L.box_sums(wq, rad))


@pytest.mark.parametrize("mode", list(MODES))
def test_determinism_split_calls_and_the_read_only_call(capi, mode):
    case = (67, 65, 3, 6, "other")
    planes, u = L.case_inputs(67, 65, 3)
    runs = []
    for split in ((6,), (6,), (2, 4), (2, "means", 4)):
        ctx = make(capi, planes, u, L.params_of("other"), mode)
        try:
            traces = []
            for n in split:
                if n == "means":
                    ctx.localized_means(6)
                else:
                    traces.append(capi.localized_run(ctx, 6, n, trace=True)[2])
            runs.append((ctx.get_levelset(), np.concatenate(traces)))
        finally:
            ctx.close()
    for other in runs[1:]:
        assert np.array_equal(bits(runs[0][0]), bits(other[0])) and np.array_equal(bits(runs[0][1]), bits(other[1]))
    assert runs[0][1].shape == L.case_reference(case)[2].shape


@pytest.mark.parametrize("sync_every,before", [(None, 0), ("k", 0), (None, 1)], ids=["inside-a-chunk", "last-of-a-chunk", "even-count"])
def test_stop_rule(capi, sync_every, before):
    """the restatement stops at iteration k: so does the card, with exactly k trace rows, and launches enqueued behind the stop change
    nothing -- the level set is that of a run with max_steps = k, bit for bit.  k is odd: the stopping call ends with its one copy of the
    level set; with `before` = 1 iteration done by an earlier call it counts k - 1, even, and ends without"""
    tol, k = L.stop_case()
    h, w, ch, rad = L.STOP_CASE
    planes, u = L.case_inputs(h, w, ch)
    a, b = (make(capi, planes, u, dict(L.DEFAULT, tol=tol)) for _ in range(2))
    try:
        stop = a.get_stop_condition()
        assert stop > 0
        if before:
            assert capi.localized_run(a, rad, before)[0] == before and capi.localized_run(b, rad, before)[0] == before
            k -= before
            assert k % 2 == 0 and k >= 2
        if sync_every:
            a.set_option("sync_every", k)
        steps, norm, trace = capi.localized_run(a, rad, 10 * k, trace=True)
        ksteps, knorm, ktrace = capi.localized_run(b, rad, k, trace=True)
        print("stop at", steps, "of", k, "norm", norm, "stop", stop)
        assert steps == k and ksteps == k and trace.shape == (k,)
        assert np.array_equal(bits(trace), bits(ktrace)) and norm == knorm
        assert norm <= stop < trace[k - 2]
        assert np.array_equal(bits(a.get_levelset()), bits(b.get_levelset()))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_means_after_a_fired_stop(capi, mode):
    """the bias-field picture of a finished run: the stop flag a run leaves in the kept workspace does not concern cvh_localized_means --
    sums == numpy's of the returned wq, every plane == that of a fresh context given the same level set, and a later run starts anew"""
    tol, k = L.stop_case()
    h, w, ch, rad = L.STOP_CASE
    planes, u = L.case_inputs(h, w, ch)
    a = make(capi, planes, u, dict(L.DEFAULT, tol=tol), mode)
    try:
        assert capi.localized_run(a, rad, 10 * k)[0] == k                     # (the stop rule fired: k < 10 k)
        m = a.localized_means(rad)
        v = a.get_levelset()
        b = make(capi, planes, v, dict(L.DEFAULT, tol=tol), mode)
        try:
            fresh = b.localized_means(rad)
        finally:
            b.close()
        c1, c2, A, S = L.means_of(planes, m["wq"], rad)
        assert np.array_equal(m["a"], A) and np.array_equal(m["s"][0], S[0])
        assert np.array_equal(bits(m["c1"][0]), bits(c1[0])) and np.array_equal(bits(m["c2"][0]), bits(c2[0]))
        assert np.abs(m["wq"].astype(np.int64) - L.weights(v).astype(np.int64)).max() <= 2
        for key in ("wq", "a", "s"):
            assert np.array_equal(m[key], fresh[key]), key
        for key in ("c1", "c2"):
            assert np.array_equal(bits(m[key]), bits(fresh[key])), key
        other = a.localized_means(rad + 1, want=("a",))["a"]                  # and at another radius, still behind the stop
        assert np.array_equal(other, L.box_sums(m["wq"], rad + 1))
        before = bits(a.get_levelset()).copy()
        assert capi.localized_run(a, rad, 2)[0] >= 1                          # a later run is not held back by the old flag
        assert not np.array_equal(bits(a.get_levelset()), before)
    finally:
        a.close()


def test_after_the_call_the_context_holds_the_new_levelset(capi):
    """every existing call sees it, and a two-phase run continued afterwards is the run after cvh_set_levelset of the same doubles"""
    h, w, ch, rad = 24, 64, 1, 4
    planes, u = L.case_inputs(h, w, ch)
    a = make(capi, planes, u, L.DEFAULT)
    f = capi.Context(h, w, ch, capi.make_params(tol=0.0))
    try:
        a.enqueue_steps(3)                                                    # (an odd count: the current buffer is the other one)
        a.sync()
        v = a.get_levelset()
        assert capi.localized_run(a, rad, 5)[0] == 5
        got = a.get_levelset()
        assert np.abs(got - L.run(planes, v, L.DEFAULT, rad, 5)[0]).max() <= L.tolerance()
        assert a.sync()[0] == 0                                               # a new run has begun
        assert np.array_equal(a.get_mask(), L.mask(got))
        f.set_image(planes)
        f.set_levelset(got)
        assert a.components(cap=0)[0] == f.components(cap=0)[0]
        la, lb = a.contours(), f.contours()
        assert len(la) == len(lb) and all(np.array_equal(x, y) for x, y in zip(la, lb))
        assert a.run(3) == f.run(3)
        assert np.array_equal(bits(a.get_levelset()), bits(f.get_levelset()))
    finally:
        a.close()
        f.close()


def test_refusals(capi):
    lib = capi.lib()
    h, w = 8, 160   # ("state" = 32 exists from 144 columns, a multiple of 16)
    planes, u = L.case_inputs(h, w, 1)
    mk = lambda: capi.Context(h, w, 1, capi.make_params(tol=0.0))
    a, state32, no_image, no_levelset = mk(), mk(), mk(), mk()
    everyone = [a, state32, no_image, no_levelset]
    try:
        for c in (a, state32, no_levelset):
            c.set_image(planes)
        for c in (a, state32, no_image):
            c.set_levelset(u)
        state32.set_option("state", 32)
        out = (C.c_double * (h * w))()
        err = lambda: lib.cvh_last_error(None).decode()
        calls = {
            "cvh_localized_run": lambda x, r: lib.cvh_localized_run(x, r, 2, None, None, None, 0, None),
            "cvh_localized_means": lambda x, r: lib.cvh_localized_means(x, r, out, None, None, None, None),
        }
        before = a.get_levelset()
        for name, call in calls.items():
            for x, r, code, text in [(a, 0, ERR_ARG, "radius = 0"), (a, 128, ERR_ARG, "radius = 128"), (a, -3, ERR_ARG, "radius = -3"),
                                     (state32, 3, ERR_ARG, 'the context has "state" = 32'), (no_image, 3, ERR_STATE, "the context has no image"),
                                     (no_levelset, 3, ERR_STATE, "the context has no level set")]:
                assert call(x._h, r) == code, (name, text, err())
                assert err().startswith(name + ": " + text), (name, text, err())
            assert call(None, 3) == ERR_ARG
        assert lib.cvh_localized_means(a._h, 3, None, None, None, None, None) == ERR_ARG and "every output is NULL" in err()
        assert lib.cvh_localized_run(a._h, 3, 2, None, None, out, -1, None) == ERR_ARG and "a trace needs" in err()
        rows = C.c_int(0)
        assert lib.cvh_localized_run(a._h, 3, 2, None, None, out, 2, None) == ERR_ARG and "a trace needs" in err()
        # NOT covered on the card: the h*w >= 2^28 refusal (a plane of 2^28 doubles is 2 GiB per buffer: no test makes one;
        # cvh_localized_geometry's zeros for that shape stand in)
        assert capi.localized_geometry(1 << 14, 1 << 14, 3)[1:] == (0, 0, 0)
        # nothing was touched, everybody is usable
        assert np.array_equal(bits(a.get_levelset()), bits(before))
        assert capi.localized_run(a, 3, 2)[0] == 2
        assert lib.cvh_localized_run(a._h, 3, 2, None, None, out, 1, C.byref(rows)) == OK and rows.value == 1
        no_levelset.set_levelset(u)
        no_image.set_image(planes)
        assert capi.localized_run(no_image, 3, 1)[0] == 1 and capi.localized_run(no_levelset, 127, 1)[0] == 1
    finally:
        for c in everyone:
            c.close()


def test_demonstration(capi):
    """the 64^2 scene: the card's mask is the restatement's on every pixel whose |u| exceeds the tolerance, and finds the disk"""
    planes, disk, u = L.demo_inputs()
    ref = L.demo_reference()
    ctx = make(capi, planes, u, L.DEMO_LOCAL)
    try:
        assert capi.localized_run(ctx, L.DEMO_RADIUS, L.DEMO_STEPS)[0] == L.DEMO_STEPS
        got, m = ctx.get_levelset(), ctx.get_mask()
    finally:
        ctx.close()
    keep = np.abs(ref) > L.tolerance()
    print("demonstration: IoU", L.iou(m, disk), "max|du|", np.abs(got - ref).max(), "pixels left out", int((~keep).sum()))
    assert np.array_equal(m[keep], L.mask(ref)[keep])
    assert L.iou(m, disk) >= 0.95
