"""Mask scores on the card (include/chanvese_hip.h, "Mask scores") against the numpy / scipy restatement (score_util.py): every field of
cvh_mask_score with ==, at the shapes of the kernels' seams -- a lane tail, one row past a band, one column past a chunk of 256 columns,
three bands --, for both channel counts and both values of invert; a member alone against the same member inside a batch; the host form
against the device form; that the calls only read; ordering against a caller's stream; every refusal."""
import ctypes as C

import numpy as np
import pytest

import score_util as S
from test_gpu_device_io import Hip

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 3
H2D, D2D = 1, 3


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    return m


@pytest.fixture()
def hip(capi):
    h = Hip()
    yield h
    h.free_all()


def launch_sets(capi):
    fn = capi.lib().cvh_debug_score_launch_sets
    fn.restype = C.c_ulong
    return fn()


def context_of(capi, name, h, w, channels, with_image=False):
    ctx = capi.Context(h, w, channels, capi.make_params(tol=0.0))
    if with_image:
        ctx.set_image(S.planes_of(h, w, channels))
    ctx.set_levelset(S.case(name, h, w)[0])
    return ctx


def raw(s):
    return bytes(s)


# ---- 1. every field, every shape, case and invert ----
@pytest.mark.parametrize("channels", S.CHANNELS)
@pytest.mark.parametrize("name", list(S.CASES))
@pytest.mark.parametrize("h,w", S.SHAPES)
def test_every_field_equals_the_restatement(capi, h, w, name, channels):
    truth = S.case(name, h, w)[1]
    with context_of(capi, name, h, w, channels) as ctx:          # an image is not required
        for invert in (False, True):
            got, want = S.as_dict(ctx.score(truth, invert=invert, tol=2.0)), S.expected(name, h, w, invert, 4)
            print(name, (h, w), channels, invert, got)
            assert got == want, (name, (h, w), invert, {k: (got[k], want[k]) for k in got if got[k] != want[k]})


def test_the_cases_cover_what_they_claim():
    """the seams are really in the data: defined / undefined cases, columns with no surface pixel, the band and chunk seams"""
    assert S.expected("truth_zero", 64, 144, False, 4)["defined"] == 0 and S.expected("truth_255", 64, 144, False, 4)["defined"] == 1
    assert S.expected("all_inside", 64, 144, False, 4)["defined"] == 1 and S.expected("all_outside", 64, 144, False, 4)["defined"] == 0
    assert S.expected("all_outside", 64, 144, True, 4)["defined"] == 1
    for h, w in S.SHAPES:
        assert S.expected("corners", h, w, False, 4)["hd2_m"] == (h - 1) ** 2 + (w - 1) ** 2
        assert S.expected("checker", h, w, False, 4)["hd2_m"] == 1
    e = S.expected("band_seam", 33, 257, False, 0)
    assert e["within_m"] == 0 and S.expected("band_seam", 33, 257, False, 1)["within_m"] == 257     # row 31 against row 32
    u, t = S.case("column_seam", 33, 257)
    assert S.surface(S.mask_of(u))[5, 255] and S.surface(t != 0)[5, 256] and not S.surface(S.mask_of(u))[5, 254]
    u, _ = S.case("mask_rule", 64, 144)
    assert np.isnan(u).any() and np.isinf(u).any() and (u == 1e-60).any() and np.signbit(u[u == 0]).any()
    assert not S.mask_of(u)[u == 1e-60].any() and not S.mask_of(u)[np.isnan(u)].any()


def test_rows_wider_than_the_lds_window(capi):
    """8200 columns: the row pass reads the distance words from global memory, a lane per column; sparse surfaces keep the all-pairs
    restatement small"""
    h, w = 3, 8200
    m, t = np.zeros((h, w), bool), np.zeros((h, w), np.uint8)
    m[:, 10:40], m[1, 8199], m[0, 4000:4100] = True, True, True
    t[1:, 25:60], t[0, 0], t[2, 8195:] = 1, 9, 255
    with capi.Context(h, w, 1) as ctx:
        ctx.set_levelset(S.levelset_of(m))
        for invert in (False, True):
            got, want = S.as_dict(ctx.score(t, invert=invert, tol=3.0)), S.score(m != invert, t != 0, 9)
            assert got == want, (invert, {k: (got[k], want[k]) for k in got if got[k] != want[k]})


# ---- 2. a batch of all shapes and both channel counts ----
def test_batch_members_equal_their_single_calls(capi, hip):
    names = list(S.CASES)
    members = [(h, w, ch, names[(3 * i + j) % len(names)]) for i, (h, w) in enumerate(S.SHAPES) for j, ch in enumerate(S.CHANNELS)]
    ctxs = [context_of(capi, name, h, w, ch, with_image=(k % 2 == 0)) for k, (h, w, ch, name) in enumerate(members)]
    try:
        truths = [hip.upload(S.case(name, h, w)[1], offset=k % 5) for k, (h, w, ch, name) in enumerate(members)]     # any byte alignment
        L = capi.lib()
        for invert in (0, 1):
            alone = []
            for c, t in zip(ctxs, truths):
                s = capi.MaskScore()
                assert L.cvh_score_mask_device(c._h, t, invert, 4, C.byref(s), None) == 0, L.cvh_last_error(None)
                alone.append(raw(s))
            before = launch_sets(capi)
            out = (capi.MaskScore * len(ctxs))()
            arr = (C.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
            ptrs = (C.c_void_p * len(ctxs))(*truths)
            assert L.cvh_score_mask_device_batch(arr, len(ctxs), ptrs, invert, 4, out, None) == 0, L.cvh_last_error(None)
            assert launch_sets(capi) == before + 1                     # ONE set of launches for the batch
            for k, (h, w, ch, name) in enumerate(members):
                assert raw(out[k]) == alone[k], (members[k], invert)
                assert S.as_dict(out[k]) == S.expected(name, h, w, bool(invert), 4), (members[k], invert)
                assert out[k].pad == 0
        # the Python driver, backwards: a member's bits do not depend on its place
        back = capi.score_batch(ctxs[::-1], truths[::-1], invert=False, tol=2.0)[::-1]
        for k, (h, w, ch, name) in enumerate(members):
            assert S.as_dict(back[k]) == S.expected(name, h, w, False, 4)
    finally:
        for c in ctxs:
            c.close()


# ---- 3. host form == device form ----
@pytest.mark.parametrize("h,w", S.SHAPES)
def test_host_form_equals_device_form(capi, hip, h, w):
    for name in ("noisy", "disks", "truth_zero"):
        truth = S.case(name, h, w)[1]
        d_truth = hip.upload(truth, offset=3)
        with context_of(capi, name, h, w, 1) as ctx:
            L = capi.lib()
            a, b = capi.MaskScore(), capi.MaskScore()
            assert L.cvh_score_mask(ctx._h, truth.ctypes.data_as(C.POINTER(C.c_uint8)), 0, 4, C.byref(a)) == 0
            assert L.cvh_score_mask_device(ctx._h, d_truth, 0, 4, C.byref(b), None) == 0
            assert raw(a) == raw(b)
            assert ctx.score(truth != 0) == ctx.score(d_truth) == ctx.score(truth)           # bool arrays, device pointers, bytes


# ---- 4. the tolerance ----
@pytest.mark.parametrize("tol2", S.TOL2S)
@pytest.mark.parametrize("h,w", S.SHAPES)
def test_tolerances(capi, h, w, tol2):
    L = capi.lib()
    for name in ("noisy", "disks", "corners", "band_seam"):
        truth = S.case(name, h, w)[1]
        with context_of(capi, name, h, w, 1) as ctx:
            s = capi.MaskScore()
            assert L.cvh_score_mask(ctx._h, truth.ctypes.data_as(C.POINTER(C.c_uint8)), 0, S.tol2_value(tol2, h, w), C.byref(s)) == 0
            want = S.expected(name, h, w, False, tol2)
            assert S.as_dict(s) == want, (name, tol2)
            if tol2 == "beyond":
                assert (s.within_m, s.within_t) == (s.surf_m, s.surf_t)


# ---- 5. read-only ----
FLAVOURS = {"per-launch": (1, {"resident": 0}), "resident": (1, {"resident": 1}), "three channels": (3, {"resident": 0}),
            "state32": (1, {"state": 32, "resident": 0})}


@pytest.mark.parametrize("in_flight", [False, True])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_score_only_reads(capi, flavour, in_flight):
    """8 iterations, the score, 8 more: level set, trace and sync() are those of a context that made the same calls but the score's;
    with the first 8 left in flight the score is of the level set behind them"""
    from chan_vese_amd import synth
    h, w = 64, 144
    channels, options = FLAVOURS[flavour]
    base = synth.disk(64, noise=24, seed=11, h=h, w=w)
    planes = [np.ascontiguousarray(np.roll(base, 5 * k, axis=1)) for k in range(channels)]
    truth = S.disk(h, w, h // 2, w // 2, 20).astype(np.uint8)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    out, seen = [], None
    for with_score in (True, False):
        with capi.Context(h, w, channels, capi.make_params(tol=0.0)) as ctx:
            for k, v in options.items():
                ctx.set_option(k, v)
            ctx.set_option("co_resident", 0)
            ctx.set_option("trace", 16)
            ctx.set_image(planes)
            ctx.init_checkerboard()
            if in_flight:
                ctx.enqueue_steps(8)
            else:
                ctx.enqueue_steps(8)
                assert ctx.sync()[0] == 8
            if with_score:
                seen = ctx.score(truth)
                assert ctx.score(truth) == seen
                assert S.as_dict(seen) == S.score(S.mask_of(ctx.get_levelset()), truth != 0, 4)
            ctx.enqueue_steps(8)
            state = ctx.sync()
            out.append((bits(ctx.get_levelset()), bits(ctx.get_trace(16)), state))
    assert out[0][2] == out[1][2] and out[0][2][0] == 16, (out[0][2], out[1][2])
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), flavour
    # the score was of the level set behind the first eight iterations
    with capi.Context(h, w, channels, capi.make_params(tol=0.0)) as ctx:
        for k, v in options.items():
            ctx.set_option(k, v)
        ctx.set_option("co_resident", 0)
        ctx.set_image(planes)
        ctx.init_checkerboard()
        ctx.enqueue_steps(8)
        assert ctx.sync()[0] == 8
        assert S.as_dict(seen) == S.score(S.mask_of(ctx.get_levelset()), truth != 0, 4)
        assert seen.defined == 1 and seen.tp > 0


# ---- 6. ordering against a caller's stream ----
def test_truth_written_on_the_callers_stream_just_before(capi, hip):
    """the truth is filled by a hipMemcpyAsync on a caller stream that is still busy behind device-to-device copies; no host wait
    between that copy and the call"""
    h, w = 96, 300
    name = "disks"
    truth = S.case(name, h, w)[1]
    stream, pin = C.c_void_p(), C.c_void_p()
    hip.ok(hip.L.hipStreamCreate(C.byref(stream)))
    hip.ok(hip.L.hipHostMalloc(C.byref(pin), truth.size, 0))
    try:
        C.memmove(pin, truth.ctypes.data, truth.size)
        big = 64 << 20
        a, b, d_truth = hip.malloc(big), hip.malloc(big), hip.malloc(truth.size)
        hip.put(d_truth, np.full(truth.size, 255, np.uint8))                 # what a call that did not wait would read
        with context_of(capi, name, h, w, 1) as ctx:
            for _ in range(6):
                hip.ok(hip.L.hipMemcpyAsync(b, a, big, D2D, stream))
            hip.ok(hip.L.hipMemcpyAsync(d_truth, pin, truth.size, H2D, stream))
            got = ctx.score(d_truth, stream=stream.value)
        assert S.as_dict(got) == S.expected(name, h, w, False, 4)
        assert S.as_dict(got) != S.expected("truth_255", h, w, False, 4)
    finally:
        hip.ok(hip.L.hipStreamSynchronize(stream))
        hip.ok(hip.L.hipStreamDestroy(stream))
        hip.ok(hip.L.hipHostFree(pin))


# ---- 7. refusals ----
def test_refusals(capi, hip):
    L = capi.lib()
    h, w = 16, 25
    mk = lambda ch=1, hh=h, ww=w: capi.Context(hh, ww, ch, capi.make_params(tol=0.0))
    ready, ready3, no_levelset, wide = mk(), mk(3), mk(), mk(1, 65536, 1)
    try:
        for c in (ready, ready3):
            c.init_checkerboard()
        wide.set_levelset(np.ones((65536, 1)))
        truth = (np.random.default_rng(2).random((h, w)) < 0.5).astype(np.uint8)
        d_t = hip.upload(truth)
        d_wide = hip.upload(np.ones((65536, 1), np.uint8))
        host_t = truth.ctypes.data_as(C.POINTER(C.c_uint8))
        before = [ready.score(d_t), ready3.score(d_t)]
        sets = launch_sets(capi)
        out = (capi.MaskScore * 4)()
        C.memset(out, 0xA5, C.sizeof(out))
        untouched = bytes(out)
        arr = lambda *cs: (C.c_void_p * max(len(cs), 1))(*[c._h.value if c is not None else None for c in cs])
        ptr = lambda *ps: (C.c_void_p * max(len(ps), 1))(*ps)
        err = lambda: L.cvh_last_error(None).decode()
        B, D, H = L.cvh_score_mask_device_batch, L.cvh_score_mask_device, L.cvh_score_mask
        cases = [
            (lambda: B(None, 2, ptr(d_t, d_t), 0, 4, out, None), ERR_ARG, "cvh_score_mask_device_batch: empty member list"),
            (lambda: B(arr(ready, ready3), 0, ptr(d_t, d_t), 0, 4, out, None), ERR_ARG, "cvh_score_mask_device_batch: empty member list"),
            (lambda: B(arr(ready, None, ready3), 3, ptr(d_t, d_t, d_t), 0, 4, out, None), ERR_ARG, "cvh_score_mask_device_batch: member 1 is NULL"),
            (lambda: B(arr(ready, ready3, ready), 3, ptr(d_t, d_t, d_t), 0, 4, out, None), ERR_ARG,
             "cvh_score_mask_device_batch: member 2 duplicates member 0"),
            (lambda: B(arr(ready, ready3), 2, ptr(d_t, d_t), 0, 4, None, None), ERR_ARG, "cvh_score_mask_device_batch: out is NULL"),
            (lambda: B(arr(ready, ready3), 2, None, 0, 4, out, None), ERR_ARG, "cvh_score_mask_device_batch: the list of device pointers is NULL"),
            (lambda: B(arr(ready, ready3), 2, ptr(d_t, None), 0, 4, out, None), ERR_ARG,
             "cvh_score_mask_device_batch: member 1: the device pointer is NULL"),
            (lambda: B(arr(ready, ready3), 2, ptr(d_t, truth.ctypes.data), 0, 4, out, None), ERR_ARG, "cvh_score_mask_device_batch: member 1: "),
            (lambda: B(arr(ready, wide), 2, ptr(d_t, d_wide), 0, 4, out, None), ERR_ARG,
             "cvh_score_mask_device_batch: member 1: 65536 x 1 is too large, h^2 + w^2 must stay below 2^32"),
            (lambda: B(arr(ready, no_levelset, ready3), 3, ptr(d_t, d_t, d_t), 0, 4, out, None), ERR_STATE,
             "cvh_score_mask_device_batch: member 1 has no level set"),
            (lambda: D(no_levelset._h, d_t, 0, 4, out, None), ERR_STATE, "cvh_score_mask_device: member 0 has no level set"),
            (lambda: D(ready._h, None, 0, 4, out, None), ERR_ARG, "cvh_score_mask_device: member 0: the device pointer is NULL"),
            (lambda: D(ready._h, d_t, 0, 4, None, None), ERR_ARG, "cvh_score_mask_device: out is NULL"),
            (lambda: D(ready._h, truth.ctypes.data, 0, 4, out, None), ERR_ARG, "cvh_score_mask_device: member 0: "),
            (lambda: H(ready._h, None, 0, 4, out), ERR_ARG, "cvh_score_mask: truth is NULL"),
            (lambda: H(ready._h, host_t, 0, 4, None), ERR_ARG, "cvh_score_mask: out is NULL"),
            (lambda: H(no_levelset._h, host_t, 0, 4, out), ERR_STATE, "cvh_score_mask: member 0 has no level set"),
        ]
        for call, code, text in cases:
            assert call() == code, (text, err())
            assert err().startswith(text), (text, err())
            assert bytes(out) == untouched, text                      # a refused call leaves `out` untouched ...
        assert "is not device-accessible memory" in (D(ready._h, truth.ctypes.data, 0, 4, out, None), err())[1]
        assert launch_sets(capi) == sets                              # ... and has launched nothing
        assert D(None, d_t, 0, 4, out, None) == ERR_ARG and H(None, host_t, 0, 4, out) == ERR_ARG
        with pytest.raises(capi.CvhError) as ex:
            capi.score_batch([ready, no_levelset], [d_t, d_t])
        assert "member 1 has no level set" in str(ex.value)
        with pytest.raises(ValueError):
            capi.score_batch([ready, ready3], [d_t])
        # everybody is as usable as before
        assert [ready.score(d_t), ready3.score(d_t)] == before == capi.score_batch([ready, ready3], [d_t, d_t])
        no_levelset.init_checkerboard()
        assert no_levelset.score(d_t) == ready.score(d_t)
    finally:
        for c in (ready, ready3, no_levelset, wide):
            c.close()
