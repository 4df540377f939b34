"""Smoothing on the GPU (cvh_smooth_planes, cvh_smooth_planes_batch) against the restatement of the header's definition
(smooth_util).  The definition is in integers, so planes, stop conditions, means, traces and level sets are compared with == (on bit
patterns for doubles).  Not covered here: the two CVH_ERR_ARG cases that no quick test can build -- contexts on different devices
(needs two GPUs) and a plane of 2^32 pixels.  Both passes make a second trip: the row pass in the large case, the column pass in the
wide one (2 x 65537: 1025 strips for a member's 1024 workgroups).  Run with -m gpu on an MI355X."""
import ctypes

import numpy as np
import pytest

import smooth_util as U
from window_util import alone, bits, device_capi, launch_sets, refusal_check, same_planes, smooth_levelset

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = 1, 3


@pytest.fixture(scope="module")
def capi():
    return device_capi()


def test_the_cases_sit_on_the_kernels_seams(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    for R in (0, 1, 20, 63):
        band, strip, segment = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        L.cvh_debug_smooth_geometry(R, ctypes.byref(band), ctypes.byref(strip), ctypes.byref(segment))
        assert (band.value, strip.value, segment.value) == (U.band_rows(R), U.STRIP, U.SEGMENT)
    assert min(U.band_rows(R) for R in range(U.RADIUS_MAX + 1)) > U.RADIUS_MAX   # no radius is as tall as its band: R = 63 stands for "R = band"
    for R in (1, 63):
        for kind in ("random", "blocky"):
            assert any(c[:3] == (U.band_rows(R) + 1, U.STRIP + 1, R) and c[4] == kind for c in U.CASES)
    h, w, R = U.WIDE[:3]
    assert U.WIDE in U.CASES and -(-h // U.band_rows(R)) * -(-w // U.STRIP) == U.BLOCKS_MAX + 1 > h * -(-w // U.SEGMENT)   # a second column trip
    assert any(c[1] == U.SEGMENT + 1 for c in U.CASES) and (5, 7, 63, "gauss", "random") in U.CASES
    assert any(c[:2] == (1, 300) for c in U.CASES) and any(c[:2] == (300, 1) for c in U.CASES)


@pytest.mark.parametrize("case", U.CASES, ids=lambda c: "%dx%d-R%d-%s-%s" % c)
def test_planes_equal_the_restatement(capi, case):
    """1 -> 1 BLUR, 1 -> 1 DETAIL, 3 -> 3 with a code per plane, 1 -> 3 (COPY, BLUR, DETAIL) and 3 -> 1, every byte"""
    h, w, R, kernel, kind = case
    taps = U.kernel_of(kernel, R)
    src1, src3 = U.planes_of(kind, h, w, 1, seed=1), U.planes_of(kind, h, w, 3, seed=2)
    with capi.Context(h, w, 1) as s1, capi.Context(h, w, 3) as s3, capi.Context(h, w, 1) as d1, capi.Context(h, w, 3) as d3:
        s1.set_image(src1)
        s3.set_image(src3)
        for what in ((U.BLUR,), (U.DETAIL,)):
            s1.smooth_planes_to(d1, taps, what)
            assert same_planes(d1.get_image(), U.expected(src1, 1, taps, what)), what
            assert same_planes(s1.get_image(), src1)
        for what in ((U.DETAIL, U.BLUR, U.COPY), (U.BLUR, U.COPY, U.DETAIL)):
            s3.smooth_planes_to(d3, taps, what)
            assert same_planes(d3.get_image(), U.expected(src3, 3, taps, what)), what
            assert same_planes(s3.get_image(), src3)
        s1.smooth_planes_to(d3, taps, (U.COPY, U.BLUR, U.DETAIL))
        assert same_planes(d3.get_image(), U.expected(src1, 3, taps, (U.COPY, U.BLUR, U.DETAIL)))
        s3.smooth_planes_to(d1, taps, (U.DETAIL,))                 # 3 -> 1: plane 0 of the source
        assert same_planes(d1.get_image(), U.expected(src3, 1, taps, (U.DETAIL,)))
        assert same_planes(s1.get_image(), src1) and same_planes(s3.get_image(), src3)


def test_large_plane_once(capi):
    h, w, R, kernel, kind = U.LARGE
    taps = U.kernel_of(kernel, R)
    src = U.planes_of(kind, h, w, 3, seed=4)
    with capi.Context(h, w, 3) as s, capi.Context(h, w, 3) as d:
        s.set_image(src)
        s.smooth_planes_to(d, taps, (U.BLUR, U.DETAIL, U.BLUR))
        assert same_planes(d.get_image(), U.expected(src, 3, taps, (U.BLUR, U.DETAIL, U.BLUR)))
        s.smooth_planes_to(d, 21.0, "blur")                        # the library's own Gaussian at its largest sigma IS these taps
        assert same_planes(d.get_image(), U.expected(src, 3, taps, (U.BLUR,) * 3))


def test_copies_alone_take_no_row_pass_and_radius_zero(capi):
    h, w = 33, 67
    src = U.planes_of("random", h, w, 3, seed=6)
    with capi.Context(h, w, 3) as s, capi.Context(h, w, 3) as d:
        s.set_image(src)
        s.smooth_planes_to(d, U.kernel_of("box", 5), (U.COPY, U.COPY, U.COPY))
        assert same_planes(d.get_image(), src)                      # (no workspace yet: a row pass would have nothing to write to)
        s.smooth_planes_to(d, [U.TAP_SUM], (U.BLUR, U.DETAIL, U.BLUR))
        assert same_planes(d.get_image(), [src[0], np.full((h, w), 128, np.uint8), src[2]])
        const = [np.full((h, w), v, np.uint8) for v in (0, 77, 255)]
        s.set_image(const)
        s.smooth_planes_to(d, 3.7, (U.BLUR, U.DETAIL, U.BLUR))
        assert same_planes(d.get_image(), [const[0], np.full((h, w), 128, np.uint8), const[2]])


def test_mixed_batch_equals_the_single_calls(capi):
    """a 1 -> 1 DETAIL pair, a 1 -> 3 (COPY, BLUR, DETAIL) pair, a 3 -> 3 pair and a 3 -> 1 BLUR pair of four shapes, radii and kernels
    in ONE call"""
    pairs = [((33, 67), 1, 1, U.kernel_of("gauss", 5), (U.DETAIL,)),
             ((U.band_rows(2) + 1, U.STRIP + 1), 1, 3, U.kernel_of("rim", 2), (U.COPY, U.BLUR, U.DETAIL)),
             ((40, 50), 3, 3, U.kernel_of("box", 63), (U.BLUR, U.COPY, U.DETAIL)), ((17, 300), 3, 1, U.kernel_of("gauss", 9), (U.BLUR,))]
    srcs = [capi.Context(*s, cs) for s, cs, _, _, _ in pairs]
    dst_b = [capi.Context(*s, cd) for s, _, cd, _, _ in pairs]
    dst_s = [capi.Context(*s, cd) for s, _, cd, _, _ in pairs]
    try:
        imgs = [U.planes_of("blocky", *s, cs, seed=i) for i, (s, cs, _, _, _) in enumerate(pairs)]
        for c, img in zip(srcs, imgs):
            c.set_image(img)
        for c in dst_b + dst_s:
            c.set_levelset(smooth_levelset(c.h, c.w))               # (the stop condition is asked of a context with a level set)
        n0 = launch_sets("smooth")
        capi.smooth_planes_batch(srcs, dst_b, [list(p[3]) for p in pairs], [p[4] for p in pairs])
        assert launch_sets("smooth") == n0 + 1                             # four pairs, ONE set of launches
        for s, d, p in zip(srcs, dst_s, pairs):
            s.smooth_planes_to(d, p[3], p[4])
        for b, s, img, p in zip(dst_b, dst_s, imgs, pairs):
            assert same_planes(b.get_image(), s.get_image()) and same_planes(b.get_image(), U.expected(img, p[2], p[3], p[4] + (0, 0)))
            assert b.get_stop_condition() == s.get_stop_condition()
        # one sigma and one name go to every pair
        capi.smooth_planes_batch(srcs[:2], dst_b[:2], 1.5, "blur")
        for b, img, p in zip(dst_b[:2], imgs[:2], pairs[:2]):
            assert same_planes(b.get_image(), U.expected(img, p[2], U.gauss_taps(1.5)[1], (U.BLUR,) * 3))
    finally:
        for c in srcs + dst_b + dst_s:
            c.close()


@pytest.mark.parametrize("channels", [1, 3])
def test_destination_equals_set_image_of_the_bytes(capi, channels):
    h, w = 33, 257
    taps = U.gauss_taps(1.5)[1]
    p = capi.make_params(tol=2.0 ** -40, lambda1=[0.25, 1, 0.5], lambda2=[0.5, 1, 0.75])   # (a power of two: equal stop conditions are equal norms)
    what = (U.COPY, U.BLUR, U.DETAIL) if channels == 3 else (U.BLUR,)
    src = U.planes_of("blocky", h, w, 1, seed=3)
    want = U.expected(src, channels, taps, what)
    with capi.Context(h, w, 1) as s, capi.Context(h, w, channels, p) as dst, capi.Context(h, w, channels, p) as control:
        s.set_image(src)
        for c in (dst, control):
            alone(c, trace=8)
            c.set_levelset(smooth_levelset(h, w))                   # before the planes arrive: kept, as cvh_set_image keeps it
        s.smooth_planes_to(dst, 1.5, what)
        control.set_image(want)
        assert same_planes(dst.get_image(), want)
        assert np.array_equal(bits(dst.get_levelset()), bits(smooth_levelset(h, w)))
        assert dst.get_stop_condition() == control.get_stop_condition()
        for c in (dst, control):
            c.init_checkerboard()
        for x, y in zip(dst.get_means(), control.get_means()):
            assert np.array_equal(bits(x), bits(y))
        ra, rb = dst.run(6), control.run(6)
        assert ra[0] == rb[0] and bits(np.float64(ra[1])) == bits(np.float64(rb[1]))
        assert np.array_equal(bits(dst.get_trace(6)), bits(control.get_trace(6)))
        assert np.array_equal(bits(dst.get_levelset()), bits(control.get_levelset()))


def test_refusals_leave_the_planes_unchanged(capi):
    h, w = 17, 19
    planes = U.planes_of("random", h, w, 3)
    with capi.Context(h, w, 3) as a, capi.Context(h, w, 3) as b, capi.Context(h, w, 3) as empty, capi.Context(h, w, 1) as one, \
            capi.Context(h, w + 1, 1) as wide, capi.Context(h, w, 1) as dst:
        for c in (a, b):
            c.set_image(planes)
        for c in (one, dst):
            c.set_image(planes[:1])
        wide.set_image([np.zeros((h, w + 1), np.uint8)])
        L = capi.lib()
        I3, T = ctypes.c_int * 3, ctypes.c_uint16 * 64
        arr = lambda *cs: (ctypes.c_void_p * len(cs))(*[c._h for c in cs])
        two = lambda x, y: (ctypes.POINTER(ctypes.c_uint16) * 2)(ctypes.cast(x, ctypes.POINTER(ctypes.c_uint16)), ctypes.cast(y, ctypes.POINTER(ctypes.c_uint16)))

        def unchanged():
            return same_planes(a.get_image(), planes) and same_planes(b.get_image(), planes) and same_planes(one.get_image(), planes[:1]) \
                and same_planes(dst.get_image(), planes[:1]) and not wide.get_image()[0].any()

        refused = refusal_check(L, unchanged)                        # (whole=: the message byte for byte)

        ok, t1 = I3(U.DETAIL, U.BLUR, U.COPY), T(16384, 8192)
        r2 = (ctypes.c_int * 2)(1, 1)
        refused(L.cvh_smooth_planes(a._h, a._h, 1, t1, ok), ERR_ARG, "cvh_smooth_planes", "pair 0")                    # src == dst
        refused(L.cvh_smooth_planes_batch(arr(a, b), arr(dst, wide), 2, r2, two(t1, t1), (ctypes.c_int * 6)()), ERR_ARG, "pair 1", f"{h} x {w}",
                whole="cvh_smooth_planes_batch: pair 1: the destination of a 17 x 19 source must be 17 x 19 too, got 17 x 20")
        wide64 = T(*([32768 - 2 * 64 * 250] + [250] * 63))
        for bad, whole in ((-1, "cvh_smooth_planes: pair 0: the radius must be 0 .. 63, got -1"),
                           (64, "cvh_smooth_planes: pair 0: the radius must be 0 .. 63, got 64")):
            refused(L.cvh_smooth_planes(a._h, dst._h, bad, wide64, ok), ERR_ARG, "pair 0", "radius", whole=whole)
        for bad, whole in ((I3(3, 0, 0), "cvh_smooth_planes: pair 0: what[0] must be CVH_SMOOTH_COPY (0), CVH_SMOOTH_BLUR (1) or CVH_SMOOTH_DETAIL (2), got 3"),
                           (I3(-1, 0, 0), "cvh_smooth_planes: pair 0: what[0] must be CVH_SMOOTH_COPY (0), CVH_SMOOTH_BLUR (1) or CVH_SMOOTH_DETAIL (2), got -1")):
            refused(L.cvh_smooth_planes(a._h, dst._h, 1, t1, bad), ERR_ARG, "pair 0", "what[0]", whole=whole)
        refused(L.cvh_smooth_planes(a._h, b._h, 1, t1, I3(0, 1, 7)), ERR_ARG, "pair 0", "what[2]")
        refused(L.cvh_smooth_planes(a._h, dst._h, 1, T(16383, 8192), ok), ERR_ARG, "pair 0",
                whole="cvh_smooth_planes: pair 0: taps[0] + 2 (taps[1] + .. + taps[1]) must be 32768, got 32767")
        refused(L.cvh_smooth_planes_batch(arr(a, b), arr(dst, one), 2, r2, two(t1, T(16384, 8193)), (ctypes.c_int * 6)()), ERR_ARG, "pair 1", "32770")
        refused(L.cvh_smooth_planes(a._h, dst._h, 1, None, ok), ERR_ARG, "pair 0", whole="cvh_smooth_planes: pair 0: its list of taps is NULL")
        refused(L.cvh_smooth_planes_batch(arr(a), arr(dst), 1, (ctypes.c_int * 1)(1), None, ok), ERR_ARG,
                whole="cvh_smooth_planes_batch: the list of tap lists is NULL")
        refused(L.cvh_smooth_planes(a._h, dst._h, 1, t1, None), ERR_ARG, whole="cvh_smooth_planes: the list of codes (what) is NULL")
        refused(L.cvh_smooth_planes_batch(arr(a), arr(dst), 0, (ctypes.c_int * 1)(1), two(t1, t1), ok), ERR_ARG, "cvh_smooth_planes_batch")
        refused(L.cvh_smooth_planes(empty._h, dst._h, 1, t1, ok), ERR_STATE, "pair 0", "no image")
        refused(L.cvh_smooth_planes_batch(arr(a, empty), arr(dst, one), 2, r2, two(t1, t1), (ctypes.c_int * 6)()), ERR_STATE, "pair 1", "no image")
        # entries of `what` behind the destination's channels are ignored, and everything stays usable
        assert L.cvh_smooth_planes(a._h, dst._h, 1, t1, I3(U.BLUR, 99, -5)) == 0
        assert same_planes(dst.get_image(), U.expected(planes, 1, (16384, 8192), (U.BLUR,)))
        a.smooth_planes_to(empty, 1.0, "detail")                     # a destination needs no image of its own
        assert same_planes(empty.get_image(), U.expected(planes, 3, U.gauss_taps(1.0)[1], (U.DETAIL,) * 3))
