"""Device-memory entry points of the C ABI against the host-buffer calls they mirror: same planes, sums, stop condition, level set,
trace and mask, BIT FOR BIT (np.array_equal / ==, no tolerance), and one ingest case per channel count against the oracle.

Device buffers are allocated without torch, through hipMalloc / hipMemcpy / hipStreamCreate of the libamdhip64 the library itself
loaded (opened by the path the process already maps, RTLD_NOLOAD: no second HIP runtime enters the process)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 3
PLANAR, INTERLEAVED = 0, 1
H2D, D2H, D2D = 1, 2, 3
# the edge shapes DESIGN.md 5 lists
SHAPES = [(1, 144), (144, 1), (3, 700), (100, 517), (150, 530), (64, 2016), (256, 256), (1080, 1920)]


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    return m


class Hip:
    """The few runtime calls the tests need, from the HIP runtime already in the process."""

    def __init__(self):
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "libchanvese_hip.so is loaded, so a libamdhip64 must be mapped"
        self.L = C.CDLL(path, mode=os.RTLD_NOLOAD | os.RTLD_NOW)
        vp, sz = C.c_void_p, C.c_size_t
        for name, args in (("hipMalloc", [C.POINTER(vp), sz]), ("hipFree", [vp]), ("hipMemcpy", [vp, vp, sz, C.c_int]),
                           ("hipMemcpyAsync", [vp, vp, sz, C.c_int, vp]), ("hipStreamCreate", [C.POINTER(vp)]),
                           ("hipStreamDestroy", [vp]), ("hipStreamSynchronize", [vp]), ("hipDeviceSynchronize", []),
                           ("hipHostMalloc", [C.POINTER(vp), sz, C.c_uint]), ("hipHostFree", [vp])):
            fn = getattr(self.L, name)
            fn.restype, fn.argtypes = C.c_int, args
        self.bufs = []

    def ok(self, rc):
        assert rc == 0, f"HIP error {rc}"

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.L.hipMalloc(C.byref(p), max(int(nbytes), 1)))
        self.bufs.append(p.value)
        return p.value

    def free_all(self):
        self.ok(self.L.hipDeviceSynchronize())
        for p in self.bufs:
            self.ok(self.L.hipFree(p))
        self.bufs = []

    def put(self, dst, arr):
        arr = np.ascontiguousarray(arr)
        self.ok(self.L.hipMemcpy(dst, arr.ctypes.data, arr.nbytes, H2D))

    def get(self, src, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        self.ok(self.L.hipMemcpy(out.ctypes.data, src, out.nbytes, D2H))
        return out

    def upload(self, arr, offset=0, slack=64):
        """arr's bytes at `offset` bytes into a fresh allocation (16-byte aligned base); returns the address of the bytes."""
        arr = np.ascontiguousarray(arr)
        base = self.malloc(arr.nbytes + offset + slack)
        self.put(base + offset, arr)
        return base + offset


@pytest.fixture()
def hip(capi):
    h = Hip()
    yield h
    h.free_all()


def rand_image(h, w, ch, seed):
    """(h, w, ch) uint8: [..., k] is plane k"""
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, ch), dtype=np.uint8)


def planes_of(img):
    return [np.ascontiguousarray(img[:, :, k]) for k in range(img.shape[2])]


def source_bytes(img, layout):
    return np.ascontiguousarray(img) if layout == INTERLEAVED else np.ascontiguousarray(img.transpose(2, 0, 1))


def same_choices(ctx):
    """Two sibling contexts are compared in bits, so neither may see the other: a context's automatic choices (data flow, strip lengths)
    look at what else lives on the device, and runs on different strips agree to 1e-9, not bit for bit."""
    ctx.set_option("co_resident", 0)
    ctx.set_option("resident", 0)


def six_iterations(ctx):
    ctx.init_checkerboard()
    means = ctx.get_means()
    done, nrm = ctx.run(6)
    return means, done, nrm, ctx.get_levelset(), ctx.get_trace(8)


def assert_same_run(a, b):
    (ma, da, na, ua, ta), (mb, db, nb, ub, tb) = a, b
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
    assert da == db and na == nb
    assert np.array_equal(ua, ub)
    assert np.array_equal(ta, tb)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ingest_equals_set_image(capi, hip, shape, channels):
    """Planar and interleaved sources at byte offsets 0, 1 and 7 into a larger allocation: the context holds the source bytes, and its stop
    condition, initial means and six iterations (level set, trace) are those of a context fed by set_image with the same bytes."""
    h, w = shape
    with capi.Context(h, w, channels) as dev, capi.Context(h, w, channels) as host:
        for ctx in (dev, host):
            ctx.set_option("trace", 8)
            same_choices(ctx)
        case = 0
        for layout in (PLANAR, INTERLEAVED):
            for off in (0, 1, 7):
                case += 1
                img = rand_image(h, w, channels, 1000 * case + h + w)
                planes = planes_of(img)
                src = hip.upload(source_bytes(img, layout), off)
                dev.set_image_device(src, layout)
                host.set_image(planes)
                got = dev.get_image()
                for k in range(channels):
                    assert np.array_equal(got[k], planes[k]), (layout, off, k)
                ref = six_iterations(host)
                run = six_iterations(dev)
                assert dev.get_stop_condition() == host.get_stop_condition(), (layout, off)
                assert_same_run(run, ref)


@pytest.mark.parametrize("channels,layout,off", [(1, PLANAR, 1), (3, INTERLEAVED, 7)])
def test_ingest_against_the_oracle(capi, hip, oracle, channels, layout, off):
    """The new entry anchored to the reference, with DESIGN.md 5's bars: stop condition equal, level set within 1e-9 max|u|, c1 / c2 / norm
    within 1e-9 relative over 10 iterations."""
    h, w = 150, 530
    img = rand_image(h, w, channels, 77 + channels)
    planes = planes_of(img)
    tol = 0.37
    with capi.Context(h, w, channels, capi.make_params(tol=tol)) as ctx:
        ctx.set_option("trace", 16)
        ctx.set_image_device(hip.upload(source_bytes(img, layout), off), layout)
        ctx.init_checkerboard()
        assert ctx.get_stop_condition() == oracle.stop_condition(planes, tol)
        ctx.set_params(capi.make_params(tol=0.0))
        done, nrm = ctx.run(10)
        u = ctx.get_levelset()
        trace = ctx.get_trace(16)
    u_cpu, done_cpu, nrm_cpu, trace_cpu = oracle.csv_run(planes, oracle.checkerboard(h, w), oracle.make_params(tol=0.0), 10)
    assert done == done_cpu == 10
    assert np.abs(u - u_cpu).max() <= 1e-9 * np.abs(u_cpu).max()
    assert abs(nrm - nrm_cpu) <= 1e-9 * nrm_cpu
    assert trace.shape == trace_cpu.shape
    assert np.all(np.abs(trace - trace_cpu) <= 1e-9 * np.abs(trace_cpu))


@pytest.mark.parametrize("state", [64, 32])
def test_levelset_in_and_out(capi, hip, state):
    """set_levelset_device (64 and 32 bits) against set_levelset (of the floats' double values); get_levelset_device 64 equals
    get_levelset(), 32 equals its astype(float32); with "state" 64 and 32; and after a run whose last iteration is still pending."""
    h, w = 320, 400
    n = h * w
    img = rand_image(h, w, 1, 5)
    rng = np.random.default_rng(9)
    u0 = rng.standard_normal((h, w)) * 3.0
    u0f = u0.astype(np.float32)
    with capi.Context(h, w, 1) as dev, capi.Context(h, w, 1) as host:
        for ctx in (dev, host):
            ctx.set_option("state", state)
            ctx.set_option("trace", 8)
            same_choices(ctx)
            ctx.set_image(planes_of(img))
        out64, out32 = hip.malloc(n * 8 + 8) + 8, hip.malloc(n * 4 + 4) + 4
        for bits, src, same in ((64, u0, u0), (32, u0f, u0f.astype(np.float64))):
            dev.set_levelset_device(hip.upload(src, bits // 8), bits)       # aligned to its element, no further (a tensor slice)
            host.set_levelset(same)
            ref = host.get_levelset()
            dev.get_levelset_device(out64, 64)
            dev.get_levelset_device(out32, 32)
            hip.ok(hip.L.hipDeviceSynchronize())
            assert np.array_equal(hip.get(out64, (h, w), np.float64), ref)
            assert np.array_equal(hip.get(out32, (h, w), np.float32), ref.astype(np.float32))
            assert np.array_equal(dev.get_levelset(), ref)
            assert np.array_equal(dev.get_means()[0], host.get_means()[0])
            a, b = dev.run(6), host.run(6)
            assert a == b and np.array_equal(dev.get_levelset(), host.get_levelset()) and np.array_equal(dev.get_trace(8), host.get_trace(8))
        # iterations enqueued and not synchronised: the getter settles them first
        for ctx in (dev, host):
            ctx.set_levelset(u0)
            ctx.enqueue_steps(5)
        dev.get_levelset_device(out64, 64)
        dev.get_levelset_device(out32, 32)
        hip.ok(hip.L.hipDeviceSynchronize())
        host.sync()
        ref = host.get_levelset()
        assert np.array_equal(hip.get(out64, (h, w), np.float64), ref)
        assert np.array_equal(hip.get(out32, (h, w), np.float32), ref.astype(np.float32))
        assert np.array_equal(dev.get_levelset(), ref)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_and_planes_out(capi, hip, shape, channels):
    """get_mask_device (invert 0 / 1) equals get_mask; get_image_device after perona_malik equals get_image(), both layouts; destinations
    at byte offsets 0, 1 and 7."""
    h, w = shape
    n = h * w
    img = rand_image(h, w, channels, 31 + h)
    with capi.Context(h, w, channels) as ctx:
        ctx.set_image(planes_of(img))
        ctx.perona_malik(30, 0.25, 1.0)
        ctx.init_checkerboard()
        ctx.run(6)
        planes = ctx.get_image()
        for off in (0, 1, 7):
            for invert in (0, 1):
                d = hip.malloc(n + 64) + off
                ctx.get_mask_device(d, invert)
                hip.ok(hip.L.hipDeviceSynchronize())
                assert np.array_equal(hip.get(d, (h, w), np.uint8), ctx.get_mask(bool(invert))), (off, invert)
            for layout in (PLANAR, INTERLEAVED):
                d = hip.malloc(n * channels + 64) + off
                ctx.get_image_device(d, layout)
                hip.ok(hip.L.hipDeviceSynchronize())
                got = hip.get(d, (h, w, channels) if layout == INTERLEAVED else (channels, h, w), np.uint8)
                for k in range(channels):
                    assert np.array_equal(got[:, :, k] if layout == INTERLEAVED else got[k], planes[k]), (off, layout, k)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("shape", [(2, 7), (1, 15), (3, 11), (5, 13)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_planes_smaller_than_or_ragged_against_a_lane(capi, hip, shape, channels):
    """Fewer than 16 pixels (byte path only) and a few pieces plus a ragged tail: ingest (planes, stop condition, initial means), mask and
    planes out against the host-buffer calls.  No iterations: only what the new kernels touch."""
    h, w = shape
    n = h * w
    with capi.Context(h, w, channels) as dev, capi.Context(h, w, channels) as host:
        for layout in (PLANAR, INTERLEAVED):
            for off in (0, 1, 7):
                img = rand_image(h, w, channels, 17 * off + layout + n)
                planes = planes_of(img)
                dev.set_image_device(hip.upload(source_bytes(img, layout), off), layout)
                host.set_image(planes)
                for k, p in enumerate(dev.get_image()):
                    assert np.array_equal(p, planes[k]), (layout, off, k)
                u0 = np.random.default_rng(off + 3).standard_normal((h, w))
                dev.set_levelset_device(hip.upload(u0, 8), 64)
                host.set_levelset(u0)
                assert dev.get_stop_condition() == host.get_stop_condition()
                a, b = dev.get_means(), host.get_means()
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                for invert in (0, 1):
                    d = hip.malloc(n + 64) + off
                    dev.get_mask_device(d, invert)
                    hip.ok(hip.L.hipDeviceSynchronize())
                    assert np.array_equal(hip.get(d, (h, w), np.uint8), host.get_mask(bool(invert)))
                d = hip.malloc(n * channels + 64) + off
                dev.get_image_device(d, layout)
                hip.ok(hip.L.hipDeviceSynchronize())
                assert np.array_equal(hip.get(d, source_bytes(img, layout).shape, np.uint8), source_bytes(img, layout))
        capi.init_checkerboard_batch([dev])
        host.init_checkerboard()
        assert np.array_equal(dev.get_levelset(), host.get_levelset())


def test_single_context_calls_refuse_bad_arguments(capi, hip):
    """The layout, bits, alignment and pointer checks of every single-context entry point, each reached with a live context."""
    h, w = 24, 40
    n = h * w
    buf = hip.malloc(8 * n + 64)
    host_mem = np.zeros(8 * n, dtype=np.uint8)
    with capi.Context(h, w, 1) as ctx:
        def refused(fn, code, text):
            with pytest.raises(capi.CvhError) as e:
                fn()
            assert e.value.code == code and text in str(e.value), str(e.value)

        for layout in (-1, 2):
            refused(lambda: ctx.set_image_device(buf, layout), ERR_ARG, "layout")
            refused(lambda: ctx.get_image_device(buf, layout), ERR_ARG, "layout")
        for bits in (0, 16, 65):
            refused(lambda: ctx.set_levelset_device(buf, bits), ERR_ARG, "bits")
            refused(lambda: ctx.get_levelset_device(buf, bits), ERR_ARG, "bits")
        refused(lambda: ctx.set_levelset_device(buf + 4, 64), ERR_ARG, "aligned")
        refused(lambda: ctx.get_levelset_device(buf + 2, 32), ERR_ARG, "aligned")
        for fn in (lambda p: ctx.set_image_device(p, PLANAR), lambda p: ctx.get_image_device(p, PLANAR), lambda p: ctx.get_mask_device(p),
                   lambda p: ctx.set_levelset_device(p, 64), lambda p: ctx.get_levelset_device(p, 32)):
            refused(lambda: fn(0), ERR_ARG, "NULL")
            refused(lambda: fn(host_mem.ctypes.data), ERR_ARG, "not device-accessible")
        refused(lambda: ctx.get_image_device(buf, PLANAR), ERR_STATE, "no image")
        refused(lambda: ctx.get_levelset_device(buf, 64), ERR_STATE, "no level set")
        refused(lambda: ctx.get_mask_device(buf), ERR_STATE, "no level set")
        # and the context is as usable as before
        img = rand_image(h, w, 1, 1)
        ctx.set_image_device(hip.upload(source_bytes(img, PLANAR)), PLANAR)
        assert np.array_equal(ctx.get_image()[0], img[:, :, 0])


def host_pipeline(capi, ctxs, imgs, steps):
    for ctx, img in zip(ctxs, imgs):
        ctx.set_image(planes_of(img))
    capi.perona_malik_batch(ctxs, 30, 0.25, 2.0)
    for ctx in ctxs:
        ctx.init_checkerboard()
    res = capi.run_batch(ctxs, steps)
    return res, [ctx.get_mask() for ctx in ctxs]


def device_pipeline(capi, hip, ctxs, imgs, steps, layout):
    srcs = [hip.upload(source_bytes(img, layout), off) for img, off in zip(imgs, (0, 1, 7, 3, 0, 5, 2, 0, 9) * 8)]
    sinks = [hip.malloc(img.shape[0] * img.shape[1] + 64) + off for img, off in zip(imgs, (0, 7, 1, 0, 3, 0, 0, 11, 2) * 8)]
    capi.set_image_device_batch(ctxs, srcs, layout)
    capi.perona_malik_batch(ctxs, 30, 0.25, 2.0)
    capi.init_checkerboard_batch(ctxs)
    res = capi.run_batch(ctxs, steps)
    capi.get_mask_device_batch(ctxs, sinks)
    hip.ok(hip.L.hipDeviceSynchronize())
    return res, [hip.get(s, img.shape[:2], np.uint8) for s, img in zip(sinks, imgs)]


def assert_batches_equal(capi, hip, specs, layout, steps=70):
    imgs = [rand_image(h, w, ch, 200 + i) // 2 + (np.indices((h, w)).sum(0)[:, :, None] % 97).astype(np.uint8) for i, (h, w, ch) in enumerate(specs)]
    dev = [capi.Context(h, w, ch) for h, w, ch in specs]
    host = [capi.Context(h, w, ch) for h, w, ch in specs]
    try:
        for ctx in dev + host:
            ctx.set_option("trace", steps)
        res_h, masks_h = host_pipeline(capi, host, imgs, steps)
        res_d, masks_d = device_pipeline(capi, hip, dev, imgs, steps, layout)
        assert res_d == res_h
        for i, (a, b) in enumerate(zip(dev, host)):
            for pa, pb in zip(a.get_image(), b.get_image()):
                assert np.array_equal(pa, pb), i
            assert np.array_equal(a.get_levelset(), b.get_levelset()), i
            assert np.array_equal(a.get_trace(steps), b.get_trace(steps)), i
            assert np.array_equal(masks_d[i], masks_h[i]), i
            assert np.array_equal(masks_d[i], a.get_mask()), i
    finally:
        for ctx in dev + host:
            ctx.close()


@pytest.mark.parametrize("layout", [PLANAR, INTERLEAVED])
def test_batch_of_mixed_members(capi, hip, layout):
    """Nine members of mixed shapes and channel counts through ingest -> Perona-Malik batch -> checkerboard batch -> run_batch(70) -> mask
    batch: planes, level set, trace and mask of every member equal those of the same member run by the host-buffer calls."""
    specs = [(256, 256, 1), (150, 530, 3), (100, 517, 1), (256, 256, 1), (64, 2016, 3), (3, 700, 1), (320, 400, 3), (144, 160, 1), (256, 256, 3)]
    assert_batches_equal(capi, hip, specs, layout)


def test_batch_of_64_small_planes(capi, hip):
    assert_batches_equal(capi, hip, [(256, 256, 1)] * 64, PLANAR)


def test_batch_errors_name_the_member_and_leave_it_usable(capi, hip):
    h, w = 96, 160
    imgs = [rand_image(h, w, 1, 40 + i) for i in range(3)]
    ctxs = [capi.Context(h, w, 1) for _ in range(3)]
    try:
        srcs = [hip.upload(source_bytes(img, PLANAR)) for img in imgs]
        sinks = [hip.malloc(h * w) for _ in imgs]
        L = capi.lib()

        def refused(fn, code, text):
            with pytest.raises(capi.CvhError) as e:
                fn()
            assert e.value.code == code and text in str(e.value), str(e.value)
            assert text.encode() in L.cvh_last_error(None)

        refused(lambda: capi.set_image_device_batch([ctxs[0], ctxs[1], ctxs[0]], srcs), ERR_ARG, "member 2 duplicates member 0")
        refused(lambda: capi.set_image_device_batch(ctxs, [srcs[0], 0, srcs[2]]), ERR_ARG, "member 1")
        refused(lambda: capi.set_image_device_batch(ctxs, srcs, 2), ERR_ARG, "layout")
        host_mem = np.zeros(h * w, dtype=np.uint8)
        refused(lambda: capi.set_image_device_batch(ctxs, [srcs[0], srcs[1], host_mem.ctypes.data]), ERR_ARG, "member 2")
        refused(lambda: capi.get_mask_device_batch(ctxs, sinks), ERR_STATE, "member 0 has no level set")
        refused(lambda: capi.init_checkerboard_batch([ctxs[0], ctxs[0]]), ERR_ARG, "member 1 duplicates member 0")
        capi.set_image_device_batch(ctxs[:2], srcs[:2])
        refused(lambda: capi.perona_malik_batch(ctxs, 30, 0.25, 1.0), ERR_STATE, "member 2")      # a member on no image
        capi.init_checkerboard_batch(ctxs[:2])
        refused(lambda: capi.get_mask_device_batch(ctxs, sinks), ERR_STATE, "member 2 has no level set")
        refused(lambda: capi.get_mask_device_batch(ctxs[:2], [sinks[0], 0]), ERR_ARG, "member 1")
        with pytest.raises(capi.CvhError) as e:
            ctxs[0].set_levelset_device(srcs[0], 16)
        assert e.value.code == ERR_ARG and "bits" in str(e.value)
        with pytest.raises(capi.CvhError) as e:
            ctxs[2].get_image_device(sinks[2], PLANAR)
        assert e.value.code == ERR_STATE
        # every member is still usable: the whole pipeline, against the host-buffer calls
        capi.set_image_device_batch(ctxs, srcs)
        capi.init_checkerboard_batch(ctxs)
        res = capi.run_batch(ctxs, 20)
        capi.get_mask_device_batch(ctxs, sinks)
        hip.ok(hip.L.hipDeviceSynchronize())
        for i, ctx in enumerate(ctxs):
            with capi.Context(h, w, 1) as ref:
                ref.set_image(planes_of(imgs[i]))
                ref.init_checkerboard()
                assert capi.run_batch([ref], 20) == [res[i]]
                assert np.array_equal(ref.get_levelset(), ctx.get_levelset())
                assert np.array_equal(ref.get_mask(), hip.get(sinks[i], (h, w), np.uint8))
    finally:
        for ctx in ctxs:
            ctx.close()


def test_ordering_against_the_callers_stream(capi, hip):
    """The source is filled by a hipMemcpyAsync on a caller stream that is still busy (behind several hundred MB of device-to-device
    copies) and the ingest follows with no host wait; the mask is consumed by a hipMemcpyAsync on that stream with no host wait after the
    call.  One pass: an ordering test, not a stress test.
    The output half is built so that a missing wait shows: the mask launch sits behind the caller's copies as well (the library's stream
    waits for what the caller's holds), so when they end, the consumer -- first in line a copy of the LAST 4 KiB of the sink, a few
    microseconds of work -- and the library's table upload + mask kernel over 3 Mpixel start together; the sink holds 0xFF, which no mask
    contains, so a consumer that does not wait for the kernel's last workgroups reads 0xFF."""
    h, w = 1536, 2048
    n = h * w
    tail = 4096
    img = rand_image(h, w, 1, 71)
    stream = C.c_void_p()
    hip.ok(hip.L.hipStreamCreate(C.byref(stream)))
    pin_src, pin_out, pin_tail = C.c_void_p(), C.c_void_p(), C.c_void_p()
    hip.ok(hip.L.hipHostMalloc(C.byref(pin_src), n, 0))
    hip.ok(hip.L.hipHostMalloc(C.byref(pin_out), n, 0))
    hip.ok(hip.L.hipHostMalloc(C.byref(pin_tail), tail, 0))
    try:
        C.memmove(pin_src.value, np.ascontiguousarray(img).ctypes.data, n)
        big = 128 << 20
        a, b = hip.malloc(big), hip.malloc(big)
        src = hip.malloc(n)
        hip.put(src, np.zeros(n, dtype=np.uint8))          # what a read that does not wait would see
        sink = hip.malloc(n)
        hip.put(sink, np.full(n, 0xFF, dtype=np.uint8))
        with capi.Context(h, w, 1) as ctx, capi.Context(h, w, 1) as ref:
            same_choices(ctx)
            same_choices(ref)
            ref.set_image(planes_of(img))
            ref.init_checkerboard()
            ref.run(12)
            for _ in range(4):                                # 512 MB of copies in front of the source's own
                hip.ok(hip.L.hipMemcpyAsync(b, a, big, D2D, stream))
            hip.ok(hip.L.hipMemcpyAsync(src, pin_src, n, H2D, stream))
            ctx.set_image_device(src, PLANAR, stream.value)
            ctx.init_checkerboard()
            ctx.run(12)
            for _ in range(2):
                hip.ok(hip.L.hipMemcpyAsync(b, a, big, D2D, stream))
            ctx.get_mask_device(sink, 0, stream.value)
            hip.ok(hip.L.hipMemcpyAsync(pin_tail, sink + n - tail, tail, D2H, stream))
            hip.ok(hip.L.hipMemcpyAsync(pin_out, sink, n, D2H, stream))
            hip.ok(hip.L.hipStreamSynchronize(stream))
            got = np.frombuffer((C.c_uint8 * n).from_address(pin_out.value), dtype=np.uint8).reshape(h, w).copy()
            got_tail = np.frombuffer((C.c_uint8 * tail).from_address(pin_tail.value), dtype=np.uint8).copy()
            assert np.array_equal(ctx.get_image()[0], img[:, :, 0])
            assert ctx.get_stop_condition() == ref.get_stop_condition()
            assert np.array_equal(ctx.get_levelset(), ref.get_levelset())
            assert np.array_equal(got_tail, ref.get_mask().reshape(-1)[n - tail:])
            assert np.array_equal(got, ref.get_mask())
    finally:
        hip.ok(hip.L.hipStreamSynchronize(stream))
        hip.ok(hip.L.hipHostFree(pin_src))
        hip.ok(hip.L.hipHostFree(pin_out))
        hip.ok(hip.L.hipHostFree(pin_tail))
        hip.ok(hip.L.hipStreamDestroy(stream))
