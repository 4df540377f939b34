"""cvh_localized_run_batch and cvh_multiphase_run_batch on the card (include/chanvese_hip.h, "Localised regions" and "Four phases"): a
member of a batch IS its own run.  Every comparison is by bit (view(uint64)) against capi.localized_run / capi.multiphase_run on fresh
contexts of the same inputs: level sets, traces, steps and norms, for mixed shapes, channel counts, radii, parameters and math modes;
in reversed order and alone; split calls; members that stop on their own; what a member is after the call; cvh_localized_means behind a
member's stop; every refusal.  The shapes are localized_util's and multiphase_util's: less than one wave-column, 61 / 62 columns,
SEGMENT + 1 columns, strips shorter than the plane, R = 127 on 2 x 2 and 9 x 300."""
import ctypes as C
import math

import numpy as np
import pytest

import localized_util as L
import multiphase_util as M
import np_restatement as R

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_STATE = 0, 1, 3
MODES = {"fast": 2, "strict": 1}
STEPS = 6

# (h, w, channels, radius, parameter set)
LOC_MEMBERS = [(67, 65, 3, 6, "other"), (5, 61, 1, 2, "default"), (3, L.SEGMENT + 1, 1, 4, "default"), (9, 300, 1, 127, "default"),
               (2, 2, 1, 127, "other")]
# multiphase_util's cases: one- and three-channel pairs mixed, every shape once
MP_MEMBERS = [c for i, c in enumerate(M.CASES) if c[:3] not in [d[:3] for d in M.CASES[:i]]]


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same(x, y):
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


def params(capi, p):
    return capi.make_params(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in p.items()})


def context(capi, planes, u, p, mode):
    ctx = capi.Context(u.shape[0], u.shape[1], len(planes), params(capi, p))
    ctx.set_option("math_mode", MODES[mode])
    ctx.set_image(planes)
    ctx.set_levelset(u)
    return ctx


def close(ctxs):
    for c in ctxs:
        if isinstance(c, tuple):
            close(c)
        else:
            c.close()


# ---- localised members
def loc_member(capi, m, mode, **over):
    h, w, ch, rad, which = m
    planes, u = L.case_inputs(h, w, ch)
    return context(capi, planes, u, dict(L.params_of(which), **over), mode)


def loc_single(capi, m, mode, steps, **over):
    """(level set, steps, norm, trace) of capi.localized_run on a fresh context: computed once per (member, mode, steps, parameters)"""
    key = ("loc", m, mode, steps, tuple(sorted(over.items())))
    if key not in _singles:
        ctx = loc_member(capi, m, mode, **over)
        try:
            done, norm, trace = capi.localized_run(ctx, m[3], steps, trace=True)
            _singles[key] = (ctx.get_levelset(), done, norm, trace)
        finally:
            ctx.close()
    return _singles[key]


_singles = {}


def loc_batch(capi, members, modes, steps, **over):
    """the members through ONE batch call: [(level set, steps, norm, trace)]"""
    ctxs = [loc_member(capi, m, mode, **over) for m, mode in zip(members, modes)]
    try:
        res = capi.localized_run_batch(ctxs, [m[3] for m in members], steps, trace=True)
        return [(c.get_levelset(), *r) for c, r in zip(ctxs, res)]
    finally:
        close(ctxs)


def assert_member(got, want, who):
    assert got[1] == want[1], (who, "steps", got[1], want[1])
    assert same(got[0], want[0]), (who, "level set")
    norms = (got[2], want[2])
    assert bits(np.array(norms[0])).tolist() == bits(np.array(norms[1])).tolist(), (who, "norm", norms)
    assert same(got[3], want[3]), (who, "trace")


def mixed(mode, n):
    """the modes of a batch's members: all `mode`, or alternating from it"""
    other = "strict" if mode == "fast" else "fast"
    return [mode] * n, [mode if i % 2 == 0 else other for i in range(n)]


@pytest.mark.parametrize("mode", list(MODES))
def test_localized_members_equal_their_own_runs(capi, mode):
    for modes in mixed(mode, len(LOC_MEMBERS)):
        got = loc_batch(capi, LOC_MEMBERS, modes, STEPS)
        for m, md, g in zip(LOC_MEMBERS, modes, got):
            assert g[1] == STEPS and g[3].shape == (STEPS,)
            assert_member(g, loc_single(capi, m, md, STEPS), (m, md))


@pytest.mark.parametrize("mode", list(MODES))
def test_localized_order_and_company_do_not_matter(capi, mode):
    modes = mixed(mode, len(LOC_MEMBERS))[1]
    got = loc_batch(capi, LOC_MEMBERS[::-1], modes[::-1], STEPS)[::-1]
    for m, md, g in zip(LOC_MEMBERS, modes, got):
        assert_member(g, loc_single(capi, m, md, STEPS), (m, md, "reversed"))
    for m in (LOC_MEMBERS[0], LOC_MEMBERS[3]):
        assert_member(loc_batch(capi, [m], [mode], STEPS)[0], loc_single(capi, m, mode, STEPS), (m, mode, "alone"))


@pytest.mark.parametrize("mode", list(MODES))
def test_localized_split_calls(capi, mode):
    ctxs = [loc_member(capi, m, mode) for m in LOC_MEMBERS]
    radii = [m[3] for m in LOC_MEMBERS]
    try:
        first = capi.localized_run_batch(ctxs, radii, 2, trace=True)
        second = capi.localized_run_batch(ctxs, radii, 4, trace=True)
        for m, c, a, b in zip(LOC_MEMBERS, ctxs, first, second):
            want = loc_single(capi, m, mode, STEPS)
            assert (a[0], b[0]) == (2, 4)
            assert same(c.get_levelset(), want[0]) and same(np.concatenate([a[2], b[2]]), want[3]), m
            assert b[1] == want[2]
    finally:
        close(ctxs)


def early_stop(worst):
    """(tol factor, k): the tol at which a run whose iteration t passes the stop rule at tol >= worst[t] stops after k iterations, 1 <= k < 6,
    with a factor of at least 1.05 on either side (the largest such k: the most iterations behind which the others go on alone)"""
    for k in range(5, 0, -1):
        before = worst[:k - 1].min() if k > 1 else math.inf
        if worst[k - 1] * 1.05 ** 2 < before:
            return (math.sqrt(worst[k - 1] * before) if k > 1 else worst[0] * 1.05), k
    raise AssertionError(f"no stopping iteration with a margin: {worst}")


@pytest.mark.parametrize("mode", list(MODES))
def test_localized_members_stop_independently(capi, mode):
    h, w, ch, rad = L.STOP_CASE
    planes, u = L.case_inputs(h, w, ch)
    tol, k = early_stop(L.run(planes, u, L.DEFAULT, rad, 5)[2] / R.stop_condition(planes, 1.0))
    assert L.run(planes, u, dict(L.DEFAULT, tol=tol), rad, 8)[1] == k and 1 <= k < 6    # the restatement stops: the test cannot pass by never stopping
    stopper, others = (h, w, ch, rad, "default"), [LOC_MEMBERS[0], LOC_MEMBERS[1]]
    ctxs = [loc_member(capi, stopper, mode, tol=tol)] + [loc_member(capi, m, mode) for m in others]
    try:
        res = capi.localized_run_batch(ctxs, [rad] + [m[3] for m in others], 8, trace=True)
        got = [(c.get_levelset(), *r) for c, r in zip(ctxs, res)]
        assert [g[1] for g in got] == [k, 8, 8]
        assert_member(got[0], loc_single(capi, stopper, mode, 8, tol=tol), "the stopped member")
        assert got[0][3].shape == (k,) and got[0][2] <= ctxs[0].get_stop_condition()
        for m, g in zip(others, got[1:]):
            assert_member(g, loc_single(capi, m, mode, 8), m)
        # cvh_localized_means behind the member's stop: what it returns after the single run (the kept stop flag does not reach it)
        means = ctxs[0].localized_means(rad)
        single = loc_member(capi, stopper, mode, tol=tol)
        try:
            assert capi.localized_run(single, rad, 8)[0] == k
            want = single.localized_means(rad)
        finally:
            single.close()
        for key in ("wq", "a", "s"):
            assert np.array_equal(means[key], want[key]), key
        for key in ("c1", "c2"):
            assert same(means[key], want[key]), key
        assert np.array_equal(means["a"], L.box_sums(means["wq"], rad))
        # and a later batch is not held back by the old flag
        assert capi.localized_run_batch(ctxs, [rad] + [m[3] for m in others], 1)[0][0] == 1
    finally:
        close(ctxs)


def test_localized_member_after_the_call(capi):
    """a two-phase run continued on a member is the run after cvh_set_levelset of the fetched doubles"""
    members = [(24, 64, 1, 4, "default"), LOC_MEMBERS[0]]
    ctxs = [loc_member(capi, m, "fast") for m in members]
    fresh = []
    try:
        ctxs[0].enqueue_steps(3)                                                    # (an odd count: the current buffer is the other one)
        ctxs[0].sync()
        assert [r[0] for r in capi.localized_run_batch(ctxs, [m[3] for m in members], 5)] == [5, 5]
        for m, c in zip(members, ctxs):
            assert c.sync()[0] == 0                                                 # a new run has begun
            planes, _ = L.case_inputs(*m[:3])
            f = context(capi, planes, c.get_levelset(), L.params_of(m[4]), "fast")
            fresh.append(f)
            assert np.array_equal(c.get_mask(), f.get_mask())
            assert c.run(3) == f.run(3)
            assert same(c.get_levelset(), f.get_levelset())
    finally:
        close(ctxs + fresh)


# ---- four-phase pairs
def mp_pair(capi, m, mode, **over):
    h, w, ch, which = m
    planes, u1, u2 = M.case_inputs(h, w, ch)
    pa, pb = M.params_of(which)
    return (context(capi, planes, u1, dict(pa, **over), mode), context(capi, planes, u2, dict(pb, **over), mode))


def mp_result(pair, r):
    return (np.stack([pair[0].get_levelset(), pair[1].get_levelset()]), r[0], np.array(r[1]), r[2])


def mp_single(capi, m, mode, steps, **over):
    key = ("mp", m, mode, steps, tuple(sorted(over.items())))
    if key not in _singles:
        pair = mp_pair(capi, m, mode, **over)
        try:
            _singles[key] = mp_result(pair, capi.multiphase_run(*pair, steps, trace=True))
        finally:
            close(pair)
    return _singles[key]


def mp_batch(capi, members, modes, steps, **over):
    pairs = [mp_pair(capi, m, mode, **over) for m, mode in zip(members, modes)]
    try:
        res = capi.multiphase_run_batch(pairs, steps, trace=True)
        return [mp_result(p, r) for p, r in zip(pairs, res)]
    finally:
        close(pairs)


@pytest.mark.parametrize("mode", list(MODES))
def test_multiphase_members_equal_their_own_runs(capi, mode):
    assert {m[2] for m in MP_MEMBERS} == {1, 3}
    for modes in mixed(mode, len(MP_MEMBERS)):
        got = mp_batch(capi, MP_MEMBERS, modes, STEPS)
        for m, md, g in zip(MP_MEMBERS, modes, got):
            assert g[1] == STEPS and g[3].shape == (STEPS, 4 * m[2] + 2)
            assert_member(g, mp_single(capi, m, md, STEPS), (m, md))


@pytest.mark.parametrize("mode", list(MODES))
def test_multiphase_order_and_company_do_not_matter(capi, mode):
    modes = mixed(mode, len(MP_MEMBERS))[1]
    got = mp_batch(capi, MP_MEMBERS[::-1], modes[::-1], STEPS)[::-1]
    for m, md, g in zip(MP_MEMBERS, modes, got):
        assert_member(g, mp_single(capi, m, md, STEPS), (m, md, "reversed"))
    for m in (MP_MEMBERS[4], MP_MEMBERS[-1]):
        assert_member(mp_batch(capi, [m], [mode], STEPS)[0], mp_single(capi, m, mode, STEPS), (m, mode, "alone"))


@pytest.mark.parametrize("mode", list(MODES))
def test_multiphase_split_calls(capi, mode):
    pairs = [mp_pair(capi, m, mode) for m in MP_MEMBERS]
    try:
        first = capi.multiphase_run_batch(pairs, 2, trace=True)
        second = capi.multiphase_run_batch(pairs, 4, trace=True)
        for m, p, a, b in zip(MP_MEMBERS, pairs, first, second):
            want = mp_single(capi, m, mode, STEPS)
            assert (a[0], b[0]) == (2, 4)
            assert same(np.stack([p[0].get_levelset(), p[1].get_levelset()]), want[0]) and same(np.concatenate([a[2], b[2]]), want[3]), m
            assert same(np.array(b[1]), want[2])
    finally:
        close(pairs)


@pytest.mark.parametrize("mode", list(MODES))
def test_multiphase_members_stop_independently(capi, mode):
    """the stop needs BOTH norms under their conditions (the same tol in both contexts: the larger norm decides)"""
    shape = M.STOP_SHAPE
    planes, u1, u2 = M.case_inputs(*shape)
    trace = M.run(planes, u1, u2, M.DEFAULT, M.DEFAULT, 5)[3]
    tol, k = early_stop(trace[:, -2:].max(axis=1) / R.stop_condition(planes, 1.0))
    p = dict(M.DEFAULT, tol=tol)
    assert M.run(planes, u1, u2, p, p, 8)[2] == k and 1 <= k < 6
    stopper, others = shape + ("default",), [MP_MEMBERS[4], MP_MEMBERS[3]]
    pairs = [mp_pair(capi, stopper, mode, tol=tol)] + [mp_pair(capi, m, mode) for m in others]
    try:
        res = capi.multiphase_run_batch(pairs, 8, trace=True)
        got = [mp_result(pr, r) for pr, r in zip(pairs, res)]
        assert [g[1] for g in got] == [k, 8, 8]
        assert_member(got[0], mp_single(capi, stopper, mode, 8, tol=tol), "the stopped pair")
        assert got[0][3].shape[0] == k and all(n <= c.get_stop_condition() for n, c in zip(got[0][2], pairs[0]))
        for m, g in zip(others, got[1:]):
            assert_member(g, mp_single(capi, m, mode, 8), m)
    finally:
        close(pairs)


def test_multiphase_member_after_the_call(capi):
    members = [(24, 64, 1, "default"), (67, 65, 3, "other")]
    pairs = [mp_pair(capi, m, "fast") for m in members]
    fresh = []
    try:
        pairs[0][1].enqueue_steps(3)                                                # (B of pair 0 alone: its current buffer is the other one)
        pairs[0][1].sync()
        assert [r[0] for r in capi.multiphase_run_batch(pairs, 5)] == [5, 5]
        for m, pair in zip(members, pairs):
            planes = M.case_inputs(*m[:3])[0]
            for c, p in zip(pair, M.params_of(m[3])):
                assert c.sync()[0] == 0
                f = context(capi, planes, c.get_levelset(), p, "fast")
                fresh.append(f)
                assert c.run(3) == f.run(3)
                assert same(c.get_levelset(), f.get_levelset())
    finally:
        close(pairs + fresh)


# ---- refusals
def handles(ctxs):
    return (C.c_void_p * max(len(ctxs), 1))(*[c._h.value if c is not None else None for c in ctxs])


def test_localized_refusals(capi):
    lib = capi.lib()
    h, w = 8, 160   # ("state" = 32 exists from 144 columns, a multiple of 16)
    planes, u = L.case_inputs(h, w, 1)
    mk = lambda: capi.Context(h, w, 1, capi.make_params(tol=0.0))
    a, b, state32, no_image, no_levelset = mk(), mk(), mk(), mk(), mk()
    everyone = [a, b, state32, no_image, no_levelset]
    try:
        for c in (a, b, state32, no_levelset):
            c.set_image(planes)
        for c in (a, b, state32, no_image):
            c.set_levelset(u)
        state32.set_option("state", 32)
        err = lambda: lib.cvh_last_error(None).decode()
        name = "cvh_localized_run_batch"

        def call(ctxs, radii, n=None, traces=None, trace_rows=0, rows=None, ctx_array=True, radius_array=True):
            n = len(ctxs) if n is None else n
            return lib.cvh_localized_run_batch(handles(ctxs) if ctx_array else None, n, (C.c_int * max(len(radii), 1))(*radii) if radius_array else None, 2,
                                               None, None, traces, trace_rows, rows)
        before = [a.get_levelset(), b.get_levelset()]
        out = (C.c_double * 4)()
        one_trace = (C.c_void_p * 2)(None, C.addressof(out))
        cases = [
            (dict(ctxs=[a, b], radii=[3, 3], n=0), ERR_ARG, "empty member list"),
            (dict(ctxs=[a, b], radii=[3, 3], n=-1), ERR_ARG, "empty member list"),
            (dict(ctxs=[a, b], radii=[3, 3], ctx_array=False), ERR_ARG, "empty member list"),
            (dict(ctxs=[a, b], radii=[3, 3], radius_array=False), ERR_ARG, "radius is NULL"),
            (dict(ctxs=[a, None], radii=[3, 3]), ERR_ARG, "member 1 is NULL"),
            (dict(ctxs=[None, a], radii=[3, 3]), ERR_ARG, "member 0 is NULL"),
            (dict(ctxs=[a, b, a], radii=[3, 3, 3]), ERR_ARG, "member 2 duplicates member 0"),
            (dict(ctxs=[a, b], radii=[3, 0]), ERR_ARG, "member 1: radius = 0"),
            (dict(ctxs=[a, b], radii=[128, 3]), ERR_ARG, "member 0: radius = 128"),
            (dict(ctxs=[a, b], radii=[3, -3]), ERR_ARG, "member 1: radius = -3"),
            (dict(ctxs=[a, b, state32], radii=[3, 3, 3]), ERR_ARG, 'member 2: the context has "state" = 32'),
            (dict(ctxs=[a, no_image, b], radii=[3, 3, 3]), ERR_STATE, "member 1: the context has no image"),
            (dict(ctxs=[a, b, no_levelset], radii=[3, 3, 3]), ERR_STATE, "member 2: the context has no level set"),
            (dict(ctxs=[a, b], radii=[3, 3], traces=one_trace, trace_rows=-1, rows=(C.c_int * 2)()), ERR_ARG, "a trace needs"),
            (dict(ctxs=[a, b], radii=[3, 3], traces=one_trace, trace_rows=2), ERR_ARG, "a trace needs"),
        ]
        for kw, code, text in cases:
            assert call(**kw) == code, (text, err())
            assert err().startswith(name + ": " + text), (text, err())
            if kw["ctxs"][0] is a and kw.get("ctx_array", True) and kw.get("n", 1) > 0:
                assert lib.cvh_last_error(a._h).decode() == err(), text   # member 0's message too
        if capi.device_count() >= 2:
            far = capi.Context(h, w, 1, capi.make_params(tol=0.0), device=1)
            everyone.append(far)
            far.set_image(planes)
            far.set_levelset(u)
            assert call([a, far], [3, 3]) == ERR_ARG and "member 1 is on device 1, member 0 on device 0" in err()
        # NOT covered on the card: the h*w >= 2^28 refusal (no test makes such a plane) and, on a machine with one device, the devices'
        # nothing was touched, everybody is usable; max_steps = 0 changes nothing and returns zeros
        assert same(a.get_levelset(), before[0]) and same(b.get_levelset(), before[1])
        assert [r[:2] for r in capi.localized_run_batch([a, b], 3, 0)] == [(0, 0.0), (0, 0.0)]
        assert same(a.get_levelset(), before[0]) and same(b.get_levelset(), before[1])
        rows = (C.c_int * 2)(7, 7)
        assert call([a, b], [3, 127], traces=one_trace, trace_rows=1, rows=rows) == OK and list(rows) == [0, 1]
    finally:
        close(everyone)


def test_multiphase_refusals(capi):
    lib = capi.lib()
    h, w = 8, 160
    planes, u1, u2 = M.case_inputs(h, w, 1)
    planes3 = M.case_inputs(h, w, 3)[0]
    mk = lambda hh=h, ww=w, ch=1, eps=1.0: capi.Context(hh, ww, ch, capi.make_params(tol=0.0, eps=eps))
    a, b, c, d, other_shape, three, other_eps, state32, no_image, no_levelset = mk(), mk(), mk(), mk(), mk(h, w + 1), mk(ch=3), mk(eps=1.5), mk(), mk(), mk()
    everyone = [a, b, c, d, other_shape, three, other_eps, state32, no_image, no_levelset]
    try:
        for x in (a, b, c, d, other_eps, state32, no_levelset):
            x.set_image(planes)
        three.set_image(planes3)
        other_shape.set_image(M.case_inputs(h, w + 1, 1)[0])
        for x in (a, c, three, other_eps, state32, no_image):
            x.set_levelset(u1)
        for x in (b, d):
            x.set_levelset(u2)
        other_shape.init_checkerboard()
        state32.set_option("state", 32)
        err = lambda: lib.cvh_last_error(None).decode()
        name = "cvh_multiphase_run_batch"

        def call(As, Bs, n=None, traces=None, trace_rows=0, rows=None, a_array=True, b_array=True):
            n = len(As) if n is None else n
            return lib.cvh_multiphase_run_batch(handles(As) if a_array else None, handles(Bs) if b_array else None, n, 2, None, None, traces, trace_rows, rows)
        everyone_before = [x.get_levelset() for x in (a, b, c, d)]
        out = (C.c_double * 16)()
        one_trace = (C.c_void_p * 2)(None, C.addressof(out))
        cases = [
            (dict(As=[a, c], Bs=[b, d], n=0), ERR_ARG, "empty pair list"),
            (dict(As=[a, c], Bs=[b, d], a_array=False), ERR_ARG, "empty pair list"),
            (dict(As=[a, c], Bs=[b, d], b_array=False), ERR_ARG, "empty pair list"),
            (dict(As=[a, None], Bs=[b, d]), ERR_ARG, "member 1: context a is NULL"),
            (dict(As=[a, c], Bs=[None, d]), ERR_ARG, "member 0: context b is NULL"),
            (dict(As=[a, c], Bs=[b, c]), ERR_ARG, "member 1: context b is also member 1's context a"),
            (dict(As=[a, c], Bs=[b, a]), ERR_ARG, "member 1: context b is also member 0's context a"),
            (dict(As=[a, b], Bs=[b, d]), ERR_ARG, "member 1: context a is also member 0's context b"),
            (dict(As=[a, c], Bs=[b, other_shape]), ERR_ARG, f"member 1: a is {h} x {w}, b {h} x {w + 1}"),
            (dict(As=[a, three], Bs=[b, d]), ERR_ARG, "member 1: a has 3 channel(s), b 1"),
            (dict(As=[a, c], Bs=[b, other_eps]), ERR_ARG, "member 1: eps must be equal"),
            (dict(As=[state32, c], Bs=[b, d]), ERR_ARG, 'member 0: context a has "state" = 32'),
            (dict(As=[a, c], Bs=[b, state32]), ERR_ARG, 'member 1: context b has "state" = 32'),
            (dict(As=[a, c], Bs=[b, no_levelset]), ERR_STATE, "member 1: context b has no level set"),
            (dict(As=[a, no_image], Bs=[b, d]), ERR_STATE, "member 1: context a has no image"),
            (dict(As=[a, c], Bs=[b, d], traces=one_trace, trace_rows=-1, rows=(C.c_int * 2)()), ERR_ARG, "a trace needs"),
            (dict(As=[a, c], Bs=[b, d], traces=one_trace, trace_rows=2), ERR_ARG, "a trace needs"),
        ]
        for kw, code, text in cases:
            assert call(**kw) == code, (text, err())
            assert err().startswith(name + ": " + text), (text, err())
            if kw["As"][0] is a and kw.get("a_array", True) and kw.get("b_array", True) and kw.get("n", 1) > 0 and kw["Bs"][0] is not None:
                assert lib.cvh_last_error(a._h).decode() == err(), text   # member 0's message too
        if capi.device_count() >= 2:
            far = [capi.Context(h, w, 1, capi.make_params(tol=0.0), device=1) for _ in range(2)]
            everyone += far
            for x, u in zip(far, (u1, u2)):
                x.set_image(planes)
                x.set_levelset(u)
            assert call([a, far[0]], [b, far[1]]) == ERR_ARG and "member 1 is on device 1, member 0 on device 0" in err()
            assert call([a, c], [b, far[1]]) == ERR_ARG and "member 1: a is on device 0, b on device 1" in err()
        for x, before in zip((a, b, c, d), everyone_before):
            assert same(x.get_levelset(), before)
        assert [(r[0], r[1]) for r in capi.multiphase_run_batch([(a, b), (c, d)], 0)] == [(0, (0.0, 0.0))] * 2
        for x, before in zip((a, b, c, d), everyone_before):
            assert same(x.get_levelset(), before)
        rows = (C.c_int * 2)(7, 7)
        assert call([a, c], [b, d], traces=one_trace, trace_rows=1, rows=rows) == OK and list(rows) == [0, 1]
    finally:
        close(everyone)
