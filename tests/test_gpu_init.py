"""Device-side initial level sets on the GPU (cvh_histogram*, cvh_otsu_threshold, cvh_init_threshold / otsu / rect / disk and their batch
forms) against the numpy / Python-integer restatement of the header's definitions (init_util).  Everything is defined in integers and
the starts select between two given doubles, so EVERY comparison is == (on bit patterns for level sets and traces); nothing here has a
tolerance.  The shapes are the smallest at which the kernels can go wrong: one pixel, one row, one column, no tail (16 x 16), an odd width
with a tail of 15 (33 x 47), a plane the 2-pixel CSV kernel takes (64 x 144), and one 2^20-pixel flat plane.  Run with -m gpu on an MI355X."""
import ctypes

import numpy as np
import pytest

import init_util as U

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def alone(ctx, **opts):
    """contexts compared in bits must not see each other in their automatic choices (tests/test_gpu_device_io.py, same_choices)"""
    ctx.set_option("co_resident", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)


def rects(h, w):
    """fully inside, clipped on each side, fully outside, covering the plane"""
    return [(w // 4, h // 4, max(w // 2, 1), max(h // 2, 1)), (-3, h // 3, 5, 2), (w - 2, 0, 7, 1), (0, -4, w, 6), (w // 2, h - 1, 1, 9),
            (w + 5, 0, 3, 3), (-9, -9, 4, 4), (-1, -1, w + 2, h + 2), (0, 0, w, h)]


def disks(h, w):
    """r = 0, the centre outside the plane, covering the plane, and an ordinary one"""
    return [(w // 2, h // 2, 0), (-3, -2, 6), (w + 4, h // 2, 9), (w // 2, h // 2, h + w), (w // 3, h // 2, max(min(h, w) // 3, 1))]


VALUES = [(1.0, -1.0), (1.0, 0.0), (NAN, 2.5), (-3.0, NAN)]


def check_start(ctx, want, planes, stop):
    """stop: the stop condition (tol = 1: the image norm) as a one-element list, empty before the first start (the getter needs a level set)"""
    got = ctx.get_levelset()
    assert np.array_equal(U.bits(got), U.bits(want))
    assert ctx.sync()[0] == 0                                         # a new run
    assert all(np.array_equal(a, b) for a, b in zip(ctx.get_image(), planes))
    if not stop:
        stop.append(ctx.get_stop_condition())
        if len(planes) == 1:                                          # one channel: the exact integer sum of squares, one IEEE sqrt
            assert stop[0] == np.sqrt(np.float64(int((planes[0].astype(np.int64) ** 2).sum())))
    assert ctx.get_stop_condition() == stop[0]
    ctx.get_means()                                                   # its precondition (an image and a level set) holds


@pytest.mark.parametrize("kind", U.KINDS)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_definitions(capi, shape, channels, kind):
    h, w = shape
    B = 255 * channels + 1
    planes = U.planes_of(kind, h, w, channels)
    want_hist = U.histogram(planes)
    with capi.Context(h, w, channels, capi.make_params(tol=1.0)) as ctx:
        ctx.set_image(planes)
        stop = []
        hist = ctx.histogram()
        assert hist.dtype == np.uint32 and hist.size == B
        assert np.array_equal(hist, want_hist)
        assert int(hist.astype(np.int64).sum()) == h * w
        assert int((np.arange(B) * hist.astype(np.int64)).sum()) == sum(int(p.astype(np.int64).sum()) for p in ctx.get_image())
        for cap in (0, 1, B - 1, B, B + 5):
            assert np.array_equal(ctx.histogram(cap), want_hist[:cap])     # a prefix
            # ... and the call itself still reports B: straight through the C ABI, with a buffer whose words past the prefix must stay
            buf = np.full(B + 8, 0xdeadbeef, dtype=np.uint32)
            bins = ctypes.c_int(-1)
            assert capi.lib().cvh_histogram(ctx._h, buf.ctypes.data if cap else None, cap, ctypes.byref(bins)) == 0
            assert bins.value == B, (cap, bins.value)
            k = min(cap, B)
            assert np.array_equal(buf[:k], want_hist[:k]) and (buf[k:] == 0xdeadbeef).all()
        assert capi.lib().cvh_histogram(ctx._h, None, 0, None) == 0           # bins is optional
        t = ctx.otsu_threshold()
        assert t == U.otsu(want_hist) == capi.otsu_from_histogram(hist)
        if kind in ("flat", "all0", "all255") or h * w == 1:
            assert t == int(np.flatnonzero(want_hist)[0])                  # the degenerate case: a single occupied bin
        for k, tt in enumerate((0, B - 1, t)):
            inside, outside = VALUES[k % len(VALUES)]
            ctx.init_threshold(tt, inside, outside)
            check_start(ctx, U.start_threshold(planes, tt, inside, outside), planes, stop)
        assert ctx.init_otsu() == t                                        # the defaults: +1 / -1
        check_start(ctx, U.start_threshold(planes, t, 1.0, -1.0), planes, stop)
        if kind in ("flat", "all0", "all255"):
            assert (ctx.get_levelset() == -1.0).all()                      # uniformly outside
        assert ctx.init_otsu(NAN, 0.0) == t
        check_start(ctx, U.start_threshold(planes, t, NAN, 0.0), planes, stop)
        for k, r in enumerate(rects(h, w)):
            inside, outside = VALUES[(k + 1) % len(VALUES)]
            ctx.init_rect(*r, inside, outside)
            check_start(ctx, U.start_rect(h, w, *r, inside, outside), planes, stop)
        for k, d in enumerate(disks(h, w)):
            inside, outside = VALUES[(k + 1) % len(VALUES)]
            ctx.init_disk(*d, inside, outside)
            check_start(ctx, U.start_disk(h, w, *d, inside, outside), planes, stop)
        ctx.init_rect(0, 0, 1, 1)                                          # the defaults: 1 / 0
        want = np.zeros((h, w)); want[0, 0] = 1.0
        assert np.array_equal(U.bits(ctx.get_levelset()), U.bits(want))
        ctx.init_disk(0, 0, 0)
        assert np.array_equal(U.bits(ctx.get_levelset()), U.bits(want))
        ctx.init_threshold(B - 1)
        assert np.array_equal(U.bits(ctx.get_levelset()), U.bits(np.full((h, w), -1.0)))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", [(33, 47), (64, 144)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_histogram_reads_the_smoothed_planes(capi, shape, channels):
    """after cvh_perona_malik the grey value is the sum of the smoothed planes: cvh_get_image's bytes"""
    h, w = shape
    planes = U.planes_of("random", h, w, channels)
    with capi.Context(h, w, channels) as ctx:
        ctx.set_image(planes)
        ctx.perona_malik(K=30, L=0.25, T=1.0)
        smooth = ctx.get_image()
        assert any(not np.array_equal(a, b) for a, b in zip(smooth, planes))
        hist = ctx.histogram()
        assert np.array_equal(hist, U.histogram(smooth))
        assert int((np.arange(hist.size) * hist.astype(np.int64)).sum()) == sum(int(p.astype(np.int64).sum()) for p in smooth)
        t = ctx.init_otsu()
        assert t == U.otsu(U.histogram(smooth))
        assert np.array_equal(U.bits(ctx.get_levelset()), U.bits(U.start_threshold(smooth, t, 1.0, -1.0)))


def test_one_flat_megapixel(capi):
    """2^20 pixels into one bin: every lane of every wave meets in one counter, and no narrow counter may wrap"""
    h = w = 1024
    with capi.Context(h, w, 1) as ctx:
        ctx.set_image([np.full((h, w), 200, dtype=np.uint8)])
        hist = ctx.histogram()
        want = np.zeros(256, dtype=np.uint32); want[200] = h * w
        assert np.array_equal(hist, want)
        assert ctx.otsu_threshold() == 200
        assert ctx.init_otsu() == 200
        assert (ctx.get_levelset() == -1.0).all()
        ctx.init_threshold(199, 4.0, NAN)
        assert (ctx.get_levelset() == 4.0).all()


def noisy(h, w, channels, seed=5):
    from chan_vese_amd import synth
    return [synth.disk(max(h, w), 200 - 30 * k, 50 + 20 * k, noise=32, seed=seed + k, h=h, w=w) for k in range(channels)]


def start_cases(h, w, planes):
    t = U.otsu(U.histogram(planes))
    r, d = (w // 5, h // 4, w // 2, h // 3), (w // 2, h // 2, min(h, w) // 3)
    return [("threshold", (t, 1.0, -1.0), U.start_threshold(planes, t, 1.0, -1.0)), ("rect", (*r, 1.0, 0.0), U.start_rect(h, w, *r, 1.0, 0.0)),
            ("disk", (*d, 1.0, 0.0), U.start_disk(h, w, *d, 1.0, 0.0))]


def iterate(ctx, k=8):
    ctx.enqueue_steps(k)
    done, nrm, _ = ctx.sync()
    return ctx.get_levelset(), ctx.get_trace(16), done, nrm


EQUIV = {"default 64x144": ((64, 144), 1, {}), "default 33x47": ((33, 47), 1, {}), "default 64x144x3": ((64, 144), 3, {}),
         "default 33x47x3": ((33, 47), 3, {}), "resident 64x144": ((64, 144), 1, {"resident": 1}), "resident 33x47": ((33, 47), 1, {"resident": 1}),
         "state 32 64x144": ((64, 144), 1, {"state": 32})}


@pytest.mark.parametrize("name", sorted(EQUIV))
def test_a_device_start_is_set_levelset(capi, name):
    """eight iterations with the trace on after a device start equal, bit for bit (level set, trace, steps, norm), eight iterations
    after cvh_set_levelset of the restated array"""
    (h, w), channels, opts = EQUIV[name]
    planes = noisy(h, w, channels)
    for kind, args, want in start_cases(h, w, planes):
        res = []
        for device in (True, False):
            with capi.Context(h, w, channels, capi.make_params(tol=0.0)) as ctx:
                alone(ctx, trace=16, **opts)
                ctx.set_image(planes)
                if device:
                    getattr(ctx, "init_" + kind)(*args)
                else:
                    ctx.set_levelset(want)
                start = ctx.get_levelset()
                res.append((start,) + iterate(ctx))
        a, b = res
        assert np.array_equal(U.bits(a[0]), U.bits(b[0])), kind
        if opts.get("state") != 32:
            assert np.array_equal(U.bits(a[0]), U.bits(want))
        assert a[3] == b[3] == 8 and a[4] == b[4], kind
        assert np.array_equal(U.bits(a[1]), U.bits(b[1])), kind
        assert a[2].shape == b[2].shape and a[2].shape[0] == 8 and np.array_equal(U.bits(a[2]), U.bits(b[2])), kind


@pytest.mark.parametrize("shape", [(64, 144), (33, 47)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_device_start_is_set_levelset_in_run_batch(capi, shape):
    """three members, one start each (batch calls), then cvh_run_batch: the members of a batch started with cvh_set_levelset"""
    h, w = shape
    planes = noisy(h, w, 1)
    cases = start_cases(h, w, planes)
    res = []
    for device in (True, False):
        ctxs = [capi.Context(h, w, 1, capi.make_params(tol=0.0)) for _ in cases]
        try:
            for ctx in ctxs:
                alone(ctx, trace=16)
                ctx.set_image(planes)
            if device:
                capi.init_threshold_batch(ctxs[:1], cases[0][1][0])
                capi.init_rect_batch(ctxs[1:2], cases[1][1][:4])
                capi.init_disk_batch(ctxs[2:], [cases[2][1][:3]])
            else:
                for ctx, (_, _, want) in zip(ctxs, cases):
                    ctx.set_levelset(want)
            done = capi.run_batch(ctxs, 8)
            res.append((done, [c.get_levelset() for c in ctxs], [c.get_trace(16) for c in ctxs]))
        finally:
            for c in ctxs:
                c.close()
    a, b = res
    assert a[0] == b[0] and [d for d, _ in a[0]] == [8, 8, 8]
    for i in range(3):
        assert np.array_equal(U.bits(a[1][i]), U.bits(b[1][i])), i
        assert a[2][i].shape[0] == 8 and np.array_equal(U.bits(a[2][i]), U.bits(b[2][i])), i


def test_a_start_in_the_middle_of_a_run_begins_a_new_run(capi):
    h, w = 64, 144
    planes = noisy(h, w, 1)
    with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx, capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ref:
        for c in (ctx, ref):
            alone(c, trace=16)
            c.set_image(planes)
        ctx.init_checkerboard()
        ctx.enqueue_steps(5)                                               # NOT synced: the start has to settle them
        t = ctx.init_otsu()
        assert ctx.sync()[0] == 0
        want = U.start_threshold(planes, t, 1.0, -1.0)
        assert np.array_equal(U.bits(ctx.get_levelset()), U.bits(want))
        ctx.enqueue_steps(3)                                               # in flight again, this time a disk
        ctx.init_disk(70, 30, 20)
        assert ctx.sync()[0] == 0
        want = U.start_disk(h, w, 70, 30, 20, 1.0, 0.0)
        assert np.array_equal(U.bits(ctx.get_levelset()), U.bits(want))
        ref.set_levelset(want)
        a, b = iterate(ctx), iterate(ref)
        assert a[2] == b[2] == 8 and a[3] == b[3]
        assert np.array_equal(U.bits(a[0]), U.bits(b[0])) and np.array_equal(U.bits(a[1]), U.bits(b[1]))


def test_a_mixed_batch_is_every_member_s_own_call(capi):
    """one call for members of mixed shapes and channel counts, each with its own parameters: byte for byte the own-call results"""
    specs = [((1, 23), 1, "random"), ((33, 47), 3, "two_valued"), ((64, 144), 1, "random")]
    ts = [100, 400, 7]
    xywh = [(3, 0, 9, 1), (-2, 5, 20, 40), (100, 10, 80, 20)]
    cxcyr = [(5, 0, 3), (50, 10, 12), (72, 32, 40)]
    imgs = [U.planes_of(kind, h, w, ch, seed=3) for (h, w), ch, kind in specs]

    def make():
        out = []
        for ((h, w), ch, _), planes in zip(specs, imgs):
            ctx = capi.Context(h, w, ch)
            ctx.set_image(planes)
            out.append(ctx)
        return out

    own, batch = make(), make()
    try:
        hists = [c.histogram() for c in own]
        got = capi.histogram_batch(batch)
        assert all(np.array_equal(a, b) and np.array_equal(a, U.histogram(p)) for a, b, p in zip(got, hists, imgs))
        got = capi.histogram_batch(batch, [256, 0, 100])                   # one member passes cap 0
        assert got[1].size == 0 and np.array_equal(got[0], hists[0]) and np.array_equal(got[2], hists[2][:100])
        assert capi.init_otsu_batch(batch, 2.0, -2.0) == [c.init_otsu(2.0, -2.0) for c in own] == [U.otsu(x) for x in hists]
        for a, b in zip(batch, own):
            assert np.array_equal(U.bits(a.get_levelset()), U.bits(b.get_levelset()))
        capi.init_threshold_batch(batch, ts, NAN, 0.5)
        for a, b, t, p in zip(batch, own, ts, imgs):
            b.init_threshold(t, NAN, 0.5)
            assert np.array_equal(U.bits(a.get_levelset()), U.bits(b.get_levelset()))
            assert np.array_equal(U.bits(a.get_levelset()), U.bits(U.start_threshold(p, t, NAN, 0.5)))
        capi.init_rect_batch(batch, xywh)
        for a, b, r in zip(batch, own, xywh):
            b.init_rect(*r)
            assert np.array_equal(U.bits(a.get_levelset()), U.bits(b.get_levelset()))
            assert np.array_equal(U.bits(a.get_levelset()), U.bits(U.start_rect(a.h, a.w, *r, 1.0, 0.0)))
        capi.init_disk_batch(batch, cxcyr, -1.0, 1.0)
        for a, b, d in zip(batch, own, cxcyr):
            b.init_disk(*d, -1.0, 1.0)
            assert np.array_equal(U.bits(a.get_levelset()), U.bits(b.get_levelset()))
            assert np.array_equal(U.bits(a.get_levelset()), U.bits(U.start_disk(a.h, a.w, *d, -1.0, 1.0)))
        capi.init_disk_batch(batch, (4, 0, 2))                             # one entry for all members
        assert all(np.array_equal(U.bits(c.get_levelset()), U.bits(U.start_disk(c.h, c.w, 4, 0, 2, 1.0, 0.0))) for c in batch)
        # the checks that need every member: nothing is launched, the level sets stay
        before = [c.get_levelset() for c in batch]
        for call, text in ((lambda: capi.init_threshold_batch(batch, [0, 766, 0]), "member 1: t must be in 0 .. 765, got 766"),
                           (lambda: capi.init_threshold_batch(batch, [0, 0, 256]), "member 2: t must be in 0 .. 255, got 256"),
                           (lambda: capi.init_threshold_batch(batch, [-1, 0, 0]), "member 0: t must be in 0 .. 255, got -1"),
                           (lambda: capi.init_rect_batch(batch, [(0, 0, 1, 1), (0, 0, 0, 1), (0, 0, 1, 1)]), "member 1: the rectangle's width and height must be positive"),
                           (lambda: capi.init_rect_batch(batch, (0, 0, 1, -1)), "member 0: the rectangle's width and height must be positive"),
                           (lambda: capi.init_disk_batch(batch, [(0, 0, 1), (0, 0, 1), (0, 0, -1)]), "member 2: the radius must not be negative"),
                           (lambda: capi.histogram_batch(batch, [256, -1, 256]), "member 1: cap must not be negative"),
                           (lambda: capi.init_otsu_batch([batch[0], batch[1], batch[0]]), "member 2 duplicates member 0")):
            with pytest.raises(capi.CvhError) as e:
                call()
            assert e.value.code == 1 and text in str(e.value)
        assert all(np.array_equal(U.bits(c.get_levelset()), U.bits(u)) for c, u in zip(batch, before))
    finally:
        for c in own + batch:
            c.close()


@pytest.mark.parametrize("channels", [1, 3])
def test_reading_calls_leave_a_run_alone(capi, channels):
    """the histogram calls and cvh_otsu_threshold only read the planes: a run continued after them is the run without them, bit for bit"""
    h, w = 64, 144
    planes = noisy(h, w, channels)
    res = []
    for reading in (True, False):
        with capi.Context(h, w, channels, capi.make_params(tol=0.0)) as ctx:
            alone(ctx, trace=16)
            ctx.set_image(planes)
            ctx.init_checkerboard()
            ctx.enqueue_steps(4)
            if reading:
                hist = ctx.histogram()                                       # settles the four iterations, as the getters do
                assert np.array_equal(hist, U.histogram(planes))
                assert ctx.otsu_threshold() == U.otsu(hist)
                assert capi.histogram_batch([ctx])[0].sum() == h * w
            assert ctx.sync()[0] == 4
            ctx.enqueue_steps(4)
            done, nrm, _ = ctx.sync()
            res.append((done, nrm, ctx.get_levelset(), ctx.get_trace(16), ctx.get_means()))
    a, b = res
    assert a[0] == b[0] == 8 and a[1] == b[1]
    assert np.array_equal(U.bits(a[2]), U.bits(b[2])) and np.array_equal(U.bits(a[3]), U.bits(b[3]))
    assert all(np.array_equal(U.bits(x), U.bits(y)) for x, y in zip(a[4], b[4]))


def test_state_errors_and_starts_without_an_image(capi):
    h, w = 33, 47
    with capi.Context(h, w, 1) as ctx, capi.Context(h, w, 3) as other:
        for call in (ctx.histogram, ctx.otsu_threshold, ctx.init_otsu, lambda: ctx.init_threshold(5)):
            with pytest.raises(capi.CvhError) as e:
                call()
            assert e.value.code == 3 and "member 0 has no image" in str(e.value)
        other.set_image(U.planes_of("random", h, w, 3))
        for call in (lambda: capi.histogram_batch([other, ctx]), lambda: capi.init_otsu_batch([other, ctx]),
                     lambda: capi.init_threshold_batch([other, ctx], 5)):
            with pytest.raises(capi.CvhError) as e:
                call()
            assert e.value.code == 3 and "member 1 has no image" in str(e.value)
        with pytest.raises(capi.CvhError) as e:
            other.get_levelset()                                           # the refused batch calls started nothing
        assert e.value.code == 3
        ctx.init_rect(5, 6, 7, 8)                                          # rect and disk need no image
        assert np.array_equal(U.bits(ctx.get_levelset()), U.bits(U.start_rect(h, w, 5, 6, 7, 8, 1.0, 0.0)))
        ctx.init_disk(20, 15, 9, 3.0, -3.0)
        assert np.array_equal(U.bits(ctx.get_levelset()), U.bits(U.start_disk(h, w, 20, 15, 9, 3.0, -3.0)))
        capi.init_disk_batch([other, ctx], [(1, 1, 1), (2, 2, 2)])
        assert np.array_equal(U.bits(other.get_levelset()), U.bits(U.start_disk(h, w, 1, 1, 1, 1.0, 0.0)))
        for call in (lambda: ctx.init_rect(0, 0, 0, 3), lambda: ctx.init_rect(0, 0, 3, -1), lambda: ctx.init_disk(0, 0, -1),
                     lambda: other.init_threshold(766), lambda: other.init_threshold(-1), lambda: other.histogram(-1)):
            with pytest.raises(capi.CvhError) as e:
                call()
            assert e.value.code == 1
        assert other.histogram(766).size == 766
