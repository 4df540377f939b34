"""Mask morphology and mask starts on the card (include/chanvese_hip.h, "Mask morphology") against the exact-integer restatement
(morph_util.py): every byte with ==, at the shapes of the kernels' seams -- a single pixel, a single row, a lane tail, one row past a
band, one column past a chunk of 256 columns, three bands --, for both channel counts, both values of invert, all five operations and
squared radii from 0 to 2^32 - 1; vertical searches across many bands; rows wider than 8192 columns; the emit launch where its lanes make a
second trip; cleaning combined with morphology; a member alone against the same member inside a batch; the host forms against the device
forms; that the byte-mask calls only read; that the level-set writes leave a context as cvh_set_levelset does; every refusal.
Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import components_util as CU
import contour_util as CT
import measure_util as MU
import morph_util as M
import trips_util as T
from test_gpu_device_io import Hip

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 3
H2D, D2D = 1, 3
NAN = float("nan")
TRIPS_MORPH_EMIT = 16                     # cvh_debug_trip_counts' code of the emit launch (debug_exports.hip)
bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


@pytest.fixture()
def hip(capi):
    h = Hip()
    yield h
    h.free_all()


def launch_sets(capi):
    fn = capi.lib().cvh_debug_morph_launch_sets
    fn.restype = C.c_ulong
    return fn()


def context_of(capi, u, channels=1, with_image=False, **options):
    h, w = u.shape
    ctx = capi.Context(h, w, channels, capi.make_params(tol=0.0))
    for k, v in options.items():
        ctx.set_option(k, v)
    if with_image:
        ctx.set_image(M.planes_of(h, w, channels))
    ctx.set_levelset(u)
    return ctx


def closing(ctxs):
    for c in ctxs:
        c.close()


def levelset_bits(f, inside, outside):
    """the bit patterns of cvh_set_levelset(where(f, inside, outside))"""
    return bits(np.where(np.asarray(f, dtype=bool), np.float64(inside), np.float64(outside)))


# ---- 1. every byte: shapes x cases x channels, and inside each invert x op x r2 ----
@pytest.mark.parametrize("channels", M.CHANNELS)
@pytest.mark.parametrize("name", list(M.CASES))
@pytest.mark.parametrize("h,w", M.SHAPES)
def test_every_byte_equals_the_restatement(capi, h, w, name, channels):
    with context_of(capi, M.case(name, h, w), channels) as ctx:      # an image is not required
        out = np.empty((h, w), np.uint8)
        for invert in (False, True):
            for op in M.OPS:
                for r2 in M.R2S:
                    out.fill(0xEE)
                    got = ctx.mask_morph(op, r2=r2, invert=invert, out=out)
                    want = M.expected(name, h, w, invert, op, r2)
                    assert np.array_equal(got, want), (name, (h, w), channels, invert, M.OP_NAMES[op], r2, int((got != want).sum()))
        assert np.array_equal(ctx.mask_morph(M.NONE, r2=25), ctx.get_mask()) and np.array_equal(ctx.mask_morph("open", radius=0.9, invert=True), ctx.get_mask(True))


# ---- 2. long vertical searches: a column's nearest set pixel is two and nine bands away, farther than 255 rows ----
@pytest.mark.parametrize("lone", ["set", "unset"])
def test_long_vertical_search(capi, lone):
    h, w = 300, 40
    f = np.zeros((h, w), bool)
    f[0, 20] = True
    if lone == "unset":
        f = ~f
    with context_of(capi, M.levelset_of(f)) as ctx:
        for r2 in (70 * 70, 299 * 299, 299 * 299 - 1, 256 * 256):
            for op in (M.DILATE, M.ERODE, M.OPEN, M.CLOSE):
                got, want = ctx.mask_morph(op, r2=r2), M.morph(f, op, r2).astype(np.uint8)
                assert np.array_equal(got, want), (lone, M.OP_NAMES[op], r2, int((got != want).sum()))
        reached = ctx.mask_morph(M.DILATE if lone == "set" else M.ERODE, r2=299 * 299)[:, 20]
        assert (reached == (1 if lone == "set" else 0)).all()        # the whole column, row 299 included


# ---- 3. rows wider than 8192 columns ----
def test_wide_rows(capi):
    h, w = 3, 8200
    f = np.zeros((h, w), bool)
    f[:, 10:40], f[1, 8199], f[0, 4000:4100], f[2, 8191:8194] = True, True, True, True
    f[1, 20] = False
    with context_of(capi, M.levelset_of(f)) as ctx:
        for invert in (False, True):
            for op in M.OPS:
                for r2 in (1, 2, 25, 100):
                    got, want = ctx.mask_morph(op, r2=r2, invert=invert), M.morph(f != invert, op, r2).astype(np.uint8)
                    assert np.array_equal(got, want), (invert, M.OP_NAMES[op], r2)


# ---- 4. the capped grid of the emit launch: its lanes make a second trip, the ragged tail alive ----
def test_emit_second_trip(capi, hip):
    """bytes out (host and device form), level set out and the mask start at the shape where the library says a lane of the emit launch
    takes a second piece; then the same member as member 1 of 3"""
    h, w = T.IO_SHAPE
    n = h * w
    assert T.trips(TRIPS_MORPH_EMIT, h, w) == 2 and n % 16 == 1
    rng = np.random.default_rng(21)
    f = M.noisy_disk(h, w)
    seam = T.first_trip(TRIPS_MORPH_EMIT, h, w) * 16                   # the first pixel of a second trip
    f.reshape(-1)[[0, seam - 1, seam, n - 1]] = [True, False, True, True]
    u = M.levelset_of(f, rng)
    want = {op: M.morph(f, op, 2).astype(np.uint8) for op in (M.OPEN, M.CLOSE)}
    small = [(33, 257, 3), (64, 144, 1)]
    with context_of(capi, u) as ctx:
        for op in want:
            assert np.array_equal(ctx.mask_morph(op, r2=2), want[op]), M.OP_NAMES[op]
        d = hip.malloc(n + 64) + 3
        ctx.mask_morph(M.OPEN, r2=2, out=d)
        hip.ok(hip.L.hipDeviceSynchronize())
        assert np.array_equal(hip.get(d, (h, w), np.uint8), want[M.OPEN])
        others = [context_of(capi, M.case("noisy", hh, ww), ch) for hh, ww, ch in small]
        try:
            ctxs = [others[0], ctx, others[1]]
            sinks = [hip.malloc(c.h * c.w + 64) + off for c, off in zip(ctxs, (1, 5, 0))]
            capi.mask_morph_batch(ctxs, sinks, M.CLOSE, r2=[1, 2, 5])
            hip.ok(hip.L.hipDeviceSynchronize())
            assert np.array_equal(hip.get(sinks[1], (h, w), np.uint8), want[M.CLOSE])
            for s, c, r2 in ((sinks[0], others[0], 1), (sinks[2], others[1], 5)):
                assert np.array_equal(hip.get(s, (c.h, c.w), np.uint8), c.mask_morph(M.CLOSE, r2=r2))
        finally:
            closing(others)
        ctx.morph_levelset(M.OPEN, r2=2, inside=NAN, outside=-0.0)
        assert np.array_equal(bits(ctx.get_levelset()), levelset_bits(want[M.OPEN], NAN, -0.0))
        # the mask start: the bytes of the closed mask, scaled so that 1, 2 and 255 all occur
        raw = want[M.CLOSE] * rng.integers(1, 256, size=(h, w), dtype=np.uint8)
        ctx.init_mask(hip.upload(raw, 1), inside=2.5, outside=NAN)
        assert np.array_equal(bits(ctx.get_levelset()), levelset_bits(want[M.CLOSE], 2.5, NAN))


# ---- 5. cleaning combined with morphology ----
CLEANINGS = [dict(min_area=6), dict(fill_holes=-1), dict(fill_holes=3, conn=8), dict(keep_largest=True), dict(min_area=4, fill_holes=5, keep_largest=True, conn=8)]


@pytest.mark.parametrize("channels", M.CHANNELS)
@pytest.mark.parametrize("name,h,w", [("noisy", 33, 257), ("disks", 64, 144), ("noisy", 96, 300), ("checker", 16, 16), ("mask_rule", 65, 31)])
def test_cleaning_then_morphology(capi, name, h, w, channels):
    """against cvh_get_mask_clean followed by the restatement (and against the restated cleaning as well)"""
    u = M.case(name, h, w)
    with context_of(capi, u, channels) as ctx:
        for invert in (False, True):
            for kw in CLEANINGS:
                cleaned = ctx.get_mask_clean(invert=invert, **kw)
                assert np.array_equal(cleaned, CU.clean(M.mask_of(u, invert), kw.get("conn", 4), kw.get("min_area", 0), kw.get("fill_holes", 0),
                                                        kw.get("keep_largest", False)))
                for op in M.OPS:
                    for r2 in (0, 1, 2, 9, 100):
                        got, want = ctx.mask_morph(op, r2=r2, invert=invert, **kw), M.morph(cleaned != 0, op, r2).astype(np.uint8)
                        assert np.array_equal(got, want), (name, invert, kw, M.OP_NAMES[op], r2)
            assert np.array_equal(ctx.mask_morph(M.NONE, r2=7, invert=invert), ctx.get_mask(invert))


# ---- 6. a batch of every shape and both channel counts, per-member radii all different ----
def batch_members():
    names = list(M.CASES)
    return [(h, w, ch, names[(3 * i + j) % len(names)]) for i, (h, w) in enumerate(M.SHAPES) for j, ch in enumerate(M.CHANNELS)]


def test_batch_members_equal_their_single_calls(capi, hip):
    members = batch_members()
    r2s = [0, 1, 2, 4, 5, 8, 9, 10, 13, 16, 25, 36, 100, 2 ** 32 - 1]
    assert len(r2s) == len(members) == len(set(r2s))
    ctxs = [context_of(capi, M.case(name, h, w), ch, with_image=(k % 2 == 0)) for k, (h, w, ch, name) in enumerate(members)]
    try:
        for op in (M.DILATE, M.ERODE, M.OPEN, M.CLOSE, M.NONE):
            for invert in (False, True):
                alone = [c.mask_morph(op, r2=r2, invert=invert) for c, r2 in zip(ctxs, r2s)]
                sinks = [hip.malloc(c.h * c.w + 64) + k % 5 for k, c in enumerate(ctxs)]           # any byte alignment
                for s, c in zip(sinks, ctxs):
                    hip.put(s, np.full(c.h * c.w, 0xFF, np.uint8))                                  # no mask holds 0xFF
                before = launch_sets(capi)
                capi.mask_morph_batch(ctxs, sinks, op, r2=r2s, invert=invert)
                assert launch_sets(capi) == before + 1                                              # ONE set of launches for the batch
                hip.ok(hip.L.hipDeviceSynchronize())
                for k, (h, w, ch, name) in enumerate(members):
                    got = hip.get(sinks[k], (h, w), np.uint8)
                    assert np.array_equal(got, alone[k]), (members[k], M.OP_NAMES[op], invert)
                    assert np.array_equal(got, M.expected(name, h, w, invert, op, r2s[k])), (members[k], M.OP_NAMES[op], invert)
                # backwards: a member's bytes do not depend on its place
                capi.mask_morph_batch(ctxs[::-1], sinks[::-1], op, r2=r2s[::-1], invert=invert)
                hip.ok(hip.L.hipDeviceSynchronize())
                for k, (h, w, ch, name) in enumerate(members):
                    assert np.array_equal(hip.get(sinks[k], (h, w), np.uint8), alone[k]), (members[k], "reversed")
        # with cleaning, and the level-set form: one set of launches, every member as its single call
        kw = dict(min_area=3, fill_holes=4, conn=8)
        alone = [c.mask_morph(M.OPEN, r2=r2, **kw) for c, r2 in zip(ctxs, r2s)]
        before = launch_sets(capi)
        capi.morph_levelset_batch(ctxs, M.OPEN, r2=r2s, inside=NAN, outside=-0.0, **kw)
        assert launch_sets(capi) == before + 1
        for k, c in enumerate(ctxs):
            assert np.array_equal(bits(c.get_levelset()), levelset_bits(alone[k], NAN, -0.0)), members[k]
            assert c.sync()[0] == 0 and not c.sync()[2]                                             # a new run: counter and stop flag cleared
        # the mask starts of the batch: every member from its own bytes
        raws = [np.random.default_rng(k).integers(0, 3, size=(c.h, c.w), dtype=np.uint8) * 127 for k, c in enumerate(ctxs)]
        before = launch_sets(capi)
        capi.init_mask_batch(ctxs, [hip.upload(r, k % 4) for k, r in enumerate(raws)], inside=-3.0, outside=NAN)
        assert launch_sets(capi) == before + 1
        for k, c in enumerate(ctxs):
            assert np.array_equal(bits(c.get_levelset()), levelset_bits(raws[k] != 0, -3.0, NAN)), members[k]
    finally:
        closing(ctxs)


# ---- 7. host form against device form, alignments, ordering against a caller's stream ----
def test_host_and_device_forms_agree_at_any_alignment(capi, hip):
    h, w = 33, 257
    with context_of(capi, M.case("noisy", h, w), 3) as ctx:
        for op, r2 in ((M.OPEN, 2), (M.CLOSE, 9), (M.ERODE, 1), (M.DILATE, 25), (M.NONE, 3)):
            host = ctx.mask_morph(op, r2=r2)
            assert np.array_equal(host, M.expected("noisy", h, w, False, op, r2))
            for off in range(5):
                base = hip.malloc(h * w + 64)
                hip.put(base, np.full(h * w + 64, 0xAB, np.uint8))
                ctx.mask_morph(op, r2=r2, out=base + off)
                hip.ok(hip.L.hipDeviceSynchronize())
                raw = hip.get(base, (h * w + 64,), np.uint8)
                assert np.array_equal(raw[off:off + h * w].reshape(h, w), host), (M.OP_NAMES[op], off)
                assert (raw[:off] == 0xAB).all() and (raw[off + h * w:] == 0xAB).all()              # nothing around is touched


def test_output_is_ordered_against_the_callers_stream(capi, hip):
    """the sink is cleared by a copy on a caller stream that is still busy behind device-to-device copies: the mask lands behind that
    copy, and a copy enqueued on the stream after the call sees the mask -- no host wait anywhere in between"""
    h, w = 96, 300
    want = M.expected("disks", h, w, False, M.CLOSE, 25)
    stream = C.c_void_p()
    hip.ok(hip.L.hipStreamCreate(C.byref(stream)))
    try:
        big = 64 << 20
        a, b, sink, copy, junk = hip.malloc(big), hip.malloc(big), hip.malloc(h * w), hip.malloc(h * w), hip.malloc(h * w)
        hip.put(junk, np.full(h * w, 0x77, np.uint8))
        with context_of(capi, M.case("disks", h, w)) as ctx:
            for _ in range(6):
                hip.ok(hip.L.hipMemcpyAsync(b, a, big, D2D, stream))
            hip.ok(hip.L.hipMemcpyAsync(sink, junk, h * w, D2D, stream))                            # a call that did not wait would be overwritten
            ctx.mask_morph(M.CLOSE, r2=25, out=sink, stream=stream.value)
            hip.ok(hip.L.hipMemcpyAsync(copy, sink, h * w, D2D, stream))
            hip.ok(hip.L.hipStreamSynchronize(stream))
            assert np.array_equal(hip.get(copy, (h, w), np.uint8), want) and np.array_equal(hip.get(sink, (h, w), np.uint8), want)
            # the mask start reads bytes the stream has only just written
            pin = C.c_void_p()
            raw = (want * 200).astype(np.uint8)
            hip.ok(hip.L.hipHostMalloc(C.byref(pin), raw.size, 0))
            try:
                C.memmove(pin, raw.ctypes.data, raw.size)
                for _ in range(6):
                    hip.ok(hip.L.hipMemcpyAsync(b, a, big, D2D, stream))
                hip.ok(hip.L.hipMemcpyAsync(sink, pin, raw.size, H2D, stream))
                ctx.init_mask(sink, inside=1.0, outside=-1.0, stream=stream.value)
                assert np.array_equal(bits(ctx.get_levelset()), levelset_bits(want, 1.0, -1.0))
            finally:
                hip.ok(hip.L.hipStreamSynchronize(stream))
                hip.ok(hip.L.hipHostFree(pin))
    finally:
        hip.ok(hip.L.hipStreamSynchronize(stream))
        hip.ok(hip.L.hipStreamDestroy(stream))


# ---- 8. the byte-mask calls only read ----
FLAVOURS = {"per-launch": (1, {"resident": 0}), "resident": (1, {"resident": 1}), "three channels": (3, {"resident": 0}),
            "state32": (1, {"state": 32, "resident": 0})}


@pytest.mark.parametrize("in_flight", [False, True])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_mask_morph_only_reads(capi, hip, flavour, in_flight):
    """8 iterations, the morphed masks (host, device, with cleaning), 8 more: level set, trace and sync() are those of a context that made
    the same calls but these; with the first 8 left in flight the masks are of the level set behind them"""
    from chan_vese_amd import synth
    h, w = 64, 144
    channels, options = FLAVOURS[flavour]
    base = synth.disk(64, noise=24, seed=11, h=h, w=w)
    planes = [np.ascontiguousarray(np.roll(base, 5 * k, axis=1)) for k in range(channels)]
    out, seen = [], None
    for with_calls in (True, False):
        with capi.Context(h, w, channels, capi.make_params(tol=0.0)) as ctx:
            for k, v in options.items():
                ctx.set_option(k, v)
            ctx.set_option("co_resident", 0)
            ctx.set_option("trace", 16)
            ctx.set_image(planes)
            ctx.init_checkerboard()
            ctx.enqueue_steps(8)
            if not in_flight:
                assert ctx.sync()[0] == 8
            if with_calls:
                seen = ctx.mask_morph(M.OPEN, r2=2)
                d = hip.malloc(h * w)
                ctx.mask_morph(M.CLOSE, r2=5, min_area=4, fill_holes=-1, out=d)
                assert np.array_equal(ctx.mask_morph(M.OPEN, r2=2), seen)
                assert np.array_equal(seen, M.morph(M.mask_of(ctx.get_levelset()), M.OPEN, 2))
            ctx.enqueue_steps(8)
            state = ctx.sync()
            out.append((bits(ctx.get_levelset()), bits(ctx.get_trace(16)), state))
    assert out[0][2] == out[1][2] and out[0][2][0] == 16, (out[0][2], out[1][2])
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), flavour


# ---- 9. cvh_morph_levelset: in place, a new run, and what the other mask calls see afterwards ----
def run_state(ctx, steps):
    ctx.enqueue_steps(steps)
    done, norm, _ = ctx.sync()
    return done, np.float64(norm).view(np.uint64), bits(ctx.get_levelset()), [bits(v) for v in ctx.get_means()]


@pytest.mark.parametrize("state", [64, 32])
@pytest.mark.parametrize("channels", M.CHANNELS)
def test_morph_levelset_is_set_levelset_of_the_restated_plane(capi, channels, state):
    from chan_vese_amd import synth
    h, w = 64, 144
    base = synth.disk(64, noise=24, seed=5, h=h, w=w)
    planes = [np.ascontiguousarray(np.roll(base, 7 * k, axis=1)) for k in range(channels)]
    u0 = M.case("disks", h, w)                                        # (a set that stays neither empty nor full: a uniform plane stops at once)
    for op, r2, kw, inside, outside in ((M.OPEN, 2, {}, NAN, -0.0), (M.CLOSE, 2, dict(min_area=5, fill_holes=3), 1.0, -1.0), (M.NONE, 4, dict(keep_largest=True), 2.0, -0.5)):
        got, want = [], []
        for morphs in (True, False):
            with capi.Context(h, w, channels, capi.make_params(tol=0.0)) as ctx:
                ctx.set_option("state", state)
                ctx.set_option("co_resident", 0)
                ctx.set_option("resident", 0)
                ctx.set_image(planes)
                ctx.set_levelset(u0)
                ctx.enqueue_steps(5)                                  # iterations in flight are settled first
                if morphs:
                    f = M.morph(ctx.mask_morph(M.NONE, **kw) != 0, op, r2)      # (settles: the set behind the five iterations)
                    ctx.morph_levelset(op, r2=r2, inside=inside, outside=outside, **kw)
                    plane = np.where(f, np.float64(inside), np.float64(outside))
                    assert ctx.sync()[0] == 0 and not ctx.sync()[2]                # a new run: counter and stop flag cleared
                    if state == 64:
                        assert np.array_equal(bits(ctx.get_levelset()), bits(plane)), M.OP_NAMES[op]
                    keep, seen = plane, bits(ctx.get_levelset())
                    if not np.isnan(inside):
                        got = run_state(ctx, 12)
                else:
                    ctx.sync()
                    ctx.set_levelset(keep)
                    # with either state: the level set is bit for bit what cvh_set_levelset of the restated plane leaves (NaN, -0.0 too)
                    assert np.array_equal(seen, bits(ctx.get_levelset())), (M.OP_NAMES[op], state)
                    if np.isnan(inside):
                        assert np.isnan(keep).any() and np.signbit(keep[keep == 0]).any()      # the triple holds both
                    if not np.isnan(inside):
                        want = run_state(ctx, 12)
        if want:
            assert got[0] == want[0] == 12 and got[1] == want[1], (M.OP_NAMES[op], got[:2], want[:2])
            assert np.array_equal(got[2], want[2]) and all(np.array_equal(a, b) for a, b in zip(got[3], want[3])), M.OP_NAMES[op]


def test_the_other_mask_calls_see_the_morphed_set(capi):
    h, w = 64, 144
    planes = M.planes_of(h, w, 3)
    with context_of(capi, M.case("noisy", h, w), 3) as ctx:
        ctx.set_image(planes)
        f = M.expected("noisy", h, w, False, M.CLOSE, 2) != 0
        ctx.morph_levelset(M.CLOSE, r2=2, inside=NAN, outside=-0.0)      # NaN is outside for the mask rule: the set is now EMPTY
        assert not ctx.get_mask().any()
        ctx.set_levelset(M.case("noisy", h, w))
        ctx.morph_levelset(M.CLOSE, r2=2, inside=0.75, outside=NAN)
        assert np.array_equal(ctx.get_mask(), f.astype(np.uint8))
        K, table = ctx.components(conn=4)
        lab, want = CU.label(f, 4)
        assert K == want.size and all(np.array_equal(table[f], want[f]) for f in want.dtype.names)
        Km, regions = ctx.measure(conn=4)
        MU.assert_tables_equal(regions, MU.measure(f, planes, 4))
        CT.assert_equal(ctx.contours(conn=8), CT.trace(f, 8, True))
        assert ctx.score(f.astype(np.uint8)).fp == 0 and ctx.score(f.astype(np.uint8)).fn == 0
        assert ctx.reinit() is not None


# ---- 10. cvh_init_mask* ----
@pytest.mark.parametrize("state", [64, 32])
def test_init_mask_is_set_levelset(capi, hip, state):
    """bytes 0, 1, 2 and 255 by "!= 0"; any alignment; host, device and batch forms agree; the context afterwards, and fifty iterations
    from it, are those of cvh_set_levelset of the same doubles"""
    from chan_vese_amd import synth
    h, w = 65, 160                                                    # ("state" = 32 takes widths that are multiples of 16 from 144 on)
    rng = np.random.default_rng(9)
    raw = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), size=(h, w))
    raw.reshape(-1)[:4] = [0, 1, 2, 255]
    planes = [synth.disk(40, noise=20, seed=2, h=h, w=w)]
    inside, outside = 1.25, -0.75
    plane = np.where(raw != 0, inside, outside)
    runs = []
    for form in ("set_levelset", "host", "bool", "device+0", "device+1", "device+3", "batch"):
        with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx, capi.Context(16, 16, 3) as other:
            ctx.set_option("state", state)
            ctx.set_option("co_resident", 0)
            ctx.set_option("resident", 0)
            ctx.set_image(planes)
            ctx.init_checkerboard()
            ctx.enqueue_steps(3)                                      # settled first
            if form == "set_levelset":
                ctx.sync()
                ctx.set_levelset(plane)
            elif form == "host":
                ctx.init_mask(raw, inside, outside)
            elif form == "bool":
                ctx.init_mask(raw != 0, inside, outside)
            elif form == "batch":
                small = np.eye(16, dtype=np.uint8) * 9
                capi.init_mask_batch([other, ctx], [hip.upload(small, 2), hip.upload(raw, 5)], inside, outside)
                assert np.array_equal(bits(other.get_levelset()), levelset_bits(small, inside, outside))
            else:
                ctx.init_mask(hip.upload(raw, int(form[-1])), inside, outside)
            assert ctx.sync()[0] == 0
            if state == 64:
                assert np.array_equal(bits(ctx.get_levelset()), bits(plane)), form
            runs.append(run_state(ctx, 50))
    for form, r in zip(("host", "bool", "device+0", "device+1", "device+3", "batch"), runs[1:]):
        assert r[0] == runs[0][0] == 50 and r[1] == runs[0][1], form
        assert np.array_equal(r[2], runs[0][2]) and all(np.array_equal(a, b) for a, b in zip(r[3], runs[0][3])), form


def test_init_mask_needs_neither_image_nor_levelset(capi, hip):
    h, w = 33, 70
    raw = (np.arange(h * w, dtype=np.uint32).reshape(h, w) % 3).astype(np.uint8)
    for channels in M.CHANNELS:
        with capi.Context(h, w, channels) as ctx:
            ctx.init_mask(raw, NAN, -0.0)
            assert np.array_equal(bits(ctx.get_levelset()), levelset_bits(raw, NAN, -0.0))
            ctx.init_mask(hip.upload(raw, 1), 3.0, -3.0)
            assert np.array_equal(ctx.get_mask(), (raw != 0).astype(np.uint8))
            assert np.array_equal(ctx.mask_morph(M.DILATE, r2=1), M.dilate(raw != 0, 1).astype(np.uint8))


# ---- 11. refusals ----
def test_refusals(capi, hip):
    L = capi.lib()
    err = lambda: L.cvh_last_error(None).decode()
    h, w = 16, 16
    u = M.case("noisy", h, w)
    host = np.zeros((h, w), np.uint8)
    hp = host.ctypes.data_as(C.POINTER(C.c_uint8))
    with context_of(capi, u) as a, context_of(capi, u, 3) as b, capi.Context(h, w, 1) as bare:
        sink = hip.malloc(h * w)
        arr = (C.c_void_p * 2)(a._h.value, b._h.value)
        arr_bare = (C.c_void_p * 2)(a._h.value, bare._h.value)
        ptrs = (C.c_void_p * 2)(sink, sink)
        r2 = (C.c_uint32 * 2)(1, 2)
        before = launch_sets(capi)
        # op outside 0 .. 4
        for op in (-1, 5):
            assert L.cvh_get_mask_morph(a._h, hp, 4, 0, 0, 0, 0, op, 1) == ERR_ARG and "op must be" in err()
            assert L.cvh_get_mask_morph_device(a._h, sink, 4, 0, 0, 0, 0, op, 1, None) == ERR_ARG
            assert L.cvh_get_mask_morph_device_batch(arr, 2, ptrs, 4, 0, 0, 0, 0, op, r2, None) == ERR_ARG
            assert L.cvh_morph_levelset(a._h, 4, 0, 0, 0, 0, op, 1, 1.0, -1.0) == ERR_ARG
            assert L.cvh_morph_levelset_batch(arr, 2, 4, 0, 0, 0, 0, op, r2, 1.0, -1.0) == ERR_ARG and "cvh_morph_levelset_batch" in err()
        # the clean-mask calls' argument errors
        for args, text in (((5, 0, 0, 0, 0), "conn must be 4 or 8"), ((4, 0, -1, 0, 0), "min_area"), ((4, 0, 0, -2, 0), "fill_holes"), ((4, 0, 0, 0, 2), "keep_largest")):
            assert L.cvh_get_mask_morph(a._h, hp, *args, 1, 1) == ERR_ARG and text in err(), text
            assert L.cvh_get_mask_morph_device_batch(arr, 2, ptrs, *args, 1, r2, None) == ERR_ARG and text in err(), text
            assert L.cvh_morph_levelset(a._h, *args, 1, 1, 1.0, -1.0) == ERR_ARG and text in err(), text
        # a NULL r2, mask or pointer array; a NULL context or list
        assert L.cvh_get_mask_morph_device_batch(arr, 2, ptrs, 4, 0, 0, 0, 0, 1, None, None) == ERR_ARG and "squared radii" in err()
        assert L.cvh_morph_levelset_batch(arr, 2, 4, 0, 0, 0, 0, 1, None, 1.0, -1.0) == ERR_ARG and "squared radii" in err()
        assert L.cvh_get_mask_morph_device_batch(arr, 2, None, 4, 0, 0, 0, 0, 1, r2, None) == ERR_ARG and "device pointers is NULL" in err()
        assert L.cvh_get_mask_morph(a._h, None, 4, 0, 0, 0, 0, 1, 1) == ERR_ARG and "mask is NULL" in err()
        assert L.cvh_get_mask_morph_device(a._h, None, 4, 0, 0, 0, 0, 1, 1, None) == ERR_ARG and "member 0" in err()
        assert L.cvh_init_mask(a._h, None, 1.0, -1.0) == ERR_ARG and "mask is NULL" in err()
        assert L.cvh_init_mask_device(a._h, None, 1.0, -1.0, None) == ERR_ARG and "member 0" in err()
        assert L.cvh_init_mask_device_batch(arr, 2, None, 1.0, -1.0, None) == ERR_ARG and "device pointers is NULL" in err()
        assert L.cvh_get_mask_morph(None, hp, 4, 0, 0, 0, 0, 1, 1) == ERR_ARG and L.cvh_init_mask(None, hp, 1.0, -1.0) == ERR_ARG
        assert L.cvh_morph_levelset(None, 4, 0, 0, 0, 0, 1, 1, 1.0, -1.0) == ERR_ARG
        assert L.cvh_get_mask_morph_device_batch(None, 2, ptrs, 4, 0, 0, 0, 0, 1, r2, None) == ERR_ARG
        assert L.cvh_init_mask_device_batch(arr, 0, ptrs, 1.0, -1.0, None) == ERR_ARG
        dup = (C.c_void_p * 2)(a._h.value, a._h.value)
        assert L.cvh_morph_levelset_batch(dup, 2, 4, 0, 0, 0, 0, 1, r2, 1.0, -1.0) == ERR_ARG and "member 1 duplicates member 0" in err()
        # a pointer that is not device memory: the member index is named
        bad = (C.c_void_p * 2)(sink, host.ctypes.data)
        assert L.cvh_get_mask_morph_device_batch(arr, 2, bad, 4, 0, 0, 0, 0, 1, r2, None) == ERR_ARG and "member 1" in err() and "not device-accessible" in err()
        assert L.cvh_init_mask_device_batch(arr, 2, bad, 1.0, -1.0, None) == ERR_ARG and "member 1" in err() and "not device-accessible" in err()
        assert L.cvh_get_mask_morph_device(a._h, host.ctypes.data, 4, 0, 0, 0, 0, 1, 1, None) == ERR_ARG and "not device-accessible" in err()
        # a member without a level set: CVH_ERR_STATE, with and without cleaning, the member index named
        for clean in (0, 3):
            assert L.cvh_get_mask_morph_device_batch(arr_bare, 2, ptrs, 4, 0, clean, 0, 0, 1, r2, None) == ERR_STATE and "member 1 has no level set" in err()
            assert L.cvh_morph_levelset_batch(arr_bare, 2, 4, 0, clean, 0, 0, 1, r2, 1.0, -1.0) == ERR_STATE and "member 1 has no level set" in err()
        assert L.cvh_get_mask_morph(bare._h, hp, 4, 0, 0, 0, 0, 1, 1) == ERR_STATE and L.cvh_morph_levelset(bare._h, 4, 0, 0, 0, 0, 1, 1, 1.0, -1.0) == ERR_STATE
        # nothing was launched, and the refused calls left the members as they were
        assert launch_sets(capi) == before
        assert np.array_equal(bits(a.get_levelset()), bits(u)) and np.array_equal(bits(b.get_levelset()), bits(u))
    # reinit's cap: h^2 + w^2 >= 2^32, the member index named (the plane itself is small)
    with capi.Context(1, 65536, 1) as wide, context_of(capi, u) as a:
        wide.init_mask(np.ones((1, 65536), np.uint8))                                              # the mask start has no such cap
        arr = (C.c_void_p * 2)(a._h.value, wide._h.value)
        r2 = (C.c_uint32 * 2)(1, 2)
        ptrs = (C.c_void_p * 2)(hip.malloc(256), hip.malloc(65536))
        assert L.cvh_get_mask_morph_device_batch(arr, 2, ptrs, 4, 0, 0, 0, 0, 1, r2, None) == ERR_ARG and "member 1" in err() and "h^2 + w^2" in err()
        assert L.cvh_morph_levelset(wide._h, 4, 0, 0, 0, 0, 1, 1, 1.0, -1.0) == ERR_ARG and "h^2 + w^2" in err()
    # the Python drivers' own checks
    with context_of(capi, u) as a:
        for bad in (dict(r2=1, radius=1.0), dict(r2=-1), dict(r2=2 ** 32), dict(radius=-0.5), dict(radius=NAN)):
            with pytest.raises(ValueError):
                a.mask_morph(M.OPEN, **bad)
        with pytest.raises(ValueError):
            a.mask_morph("shrink", r2=1)
        with pytest.raises(ValueError):
            capi.mask_morph_batch([a], [0], M.OPEN, r2=[1, 2])
