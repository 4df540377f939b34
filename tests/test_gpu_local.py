"""Local statistics on the GPU (cvh_local_planes, cvh_local_planes_batch) against the restatement of the header's definition
(local_util).  The definition is in integers, so planes, stop conditions, means, traces and level sets are compared with == (on bit
patterns for doubles); only the proposition's run against the CPU oracle has a bar, the mask bar tests/test_gpu_parity.py states.  Not covered here: the two CVH_ERR_ARG cases that no quick test can build -- contexts on different devices
(needs two GPUs) and a plane of 2^32 pixels -- and a second trip of the column pass, which takes a plane of more than 2^25 pixels (the
row pass makes its second trip in the large case).  Run with -m gpu on an MI355X."""
import ctypes

import numpy as np
import pytest

import local_util as U
from window_util import alone, bits, device_capi, launch_sets, refusal_check, same_planes, smooth_levelset

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = 1, 3


@pytest.fixture(scope="module")
def capi():
    return device_capi()


@pytest.mark.parametrize("case", U.CASES, ids=lambda c: "%dx%d-R%d-%s" % c)
def test_planes_equal_the_restatement(capi, case):
    """1 -> 1 MEAN, 1 -> 1 DEV, the 1 -> 3 stack and a 3 -> 3 pair with a code per plane, every byte"""
    h, w, R, kind = case
    src1, src3 = U.planes_of(kind, h, w, 1, seed=1), U.planes_of(kind, h, w, 3, seed=2)
    with capi.Context(h, w, 1) as s1, capi.Context(h, w, 3) as s3, capi.Context(h, w, 1) as d1, capi.Context(h, w, 3) as d3:
        s1.set_image(src1)
        s3.set_image(src3)
        for what in ((U.MEAN,), (U.DEV,)):
            s1.local_planes_to(d1, R, what)
            assert same_planes(d1.get_image(), U.expected(src1, 1, R, what)), what
        s1.local_planes_to(d3, R, "stack")
        assert same_planes(d3.get_image(), U.expected(src1, 3, R, U.STACK))
        for what in ((U.DEV, U.MEAN, U.COPY), (U.MEAN, U.COPY, U.DEV)):
            s3.local_planes_to(d3, R, what)
            assert same_planes(d3.get_image(), U.expected(src3, 3, R, what)), what
        s3.local_planes_to(d1, R, (U.DEV,))                     # 3 -> 1: plane 0 of the source
        assert same_planes(d1.get_image(), U.expected(src3, 1, R, (U.DEV,)))
        assert same_planes(s1.get_image(), src1) and same_planes(s3.get_image(), src3)


def test_large_plane_once(capi):
    h, w, R, kind = U.LARGE
    src = U.planes_of(kind, h, w, 1, seed=4)
    with capi.Context(h, w, 1) as s, capi.Context(h, w, 3) as d:
        s.set_image(src)
        s.local_planes_to(d, R, "stack")
        assert same_planes(d.get_image(), U.expected(src, 3, R, U.STACK))


def test_copies_alone_take_no_row_pass_and_radius_zero(capi):
    h, w = 33, 67
    src = U.random_planes(h, w, 3, seed=6)
    with capi.Context(h, w, 3) as s, capi.Context(h, w, 3) as d:
        s.set_image(src)
        s.local_planes_to(d, 5, (U.COPY, U.COPY, U.COPY))
        assert same_planes(d.get_image(), src)
        s.local_planes_to(d, 0, (U.MEAN, U.DEV, U.MEAN))
        assert same_planes(d.get_image(), [src[0], np.zeros((h, w), np.uint8), src[2]])


def test_mixed_batch_equals_the_single_calls(capi):
    """a 1 -> 1 DEV pair, a 1 -> 3 stack, a 3 -> 3 (MEAN, COPY, DEV) pair and a 3 -> 1 MEAN pair of four shapes and radii in ONE call"""
    pairs = [((33, 67), 1, 1, 5, (U.DEV,)), ((U.BAND + 1, U.STRIP + 1), 1, 3, 2, U.STACK), ((40, 50), 3, 3, 127, (U.MEAN, U.COPY, U.DEV)),
             ((17, 300), 3, 1, 9, (U.MEAN,))]
    srcs = [capi.Context(*s, cs) for s, cs, _, _, _ in pairs]
    dst_b = [capi.Context(*s, cd) for s, _, cd, _, _ in pairs]
    dst_s = [capi.Context(*s, cd) for s, _, cd, _, _ in pairs]
    try:
        imgs = [U.blocky_planes(*s, cs, seed=i) for i, (s, cs, _, _, _) in enumerate(pairs)]
        for c, img in zip(srcs, imgs):
            c.set_image(img)
        for c in dst_b + dst_s:
            c.set_levelset(smooth_levelset(c.h, c.w))               # (the stop condition is asked of a context with a level set)
        n0 = launch_sets("local")
        capi.local_planes_batch(srcs, dst_b, [p[3] for p in pairs], [p[4] for p in pairs])
        assert launch_sets("local") == n0 + 1                              # four pairs, ONE set of launches
        for s, d, p in zip(srcs, dst_s, pairs):
            s.local_planes_to(d, p[3], p[4])
        for b, s, img, p in zip(dst_b, dst_s, imgs, pairs):
            assert same_planes(b.get_image(), s.get_image()) and same_planes(b.get_image(), U.expected(img, p[2], p[3], p[4] + (0, 0)))
            assert b.get_stop_condition() == s.get_stop_condition()
        # a scalar radius and one tuple of codes go to every pair
        capi.local_planes_batch(srcs[:2], dst_b[:2], 3, "dev")
        for b, img, p in zip(dst_b[:2], imgs[:2], pairs[:2]):
            assert same_planes(b.get_image(), U.expected(img, p[2], 3, (U.DEV,) * 3))
    finally:
        for c in srcs + dst_b + dst_s:
            c.close()


@pytest.mark.parametrize("channels", [1, 3])
def test_destination_equals_set_image_of_the_bytes(capi, channels):
    h, w, R = 33, 257, 4
    p = capi.make_params(tol=2.0 ** -40, lambda1=[0.25, 1, 0.5], lambda2=[0.5, 1, 0.75])   # (a power of two: equal stop conditions are equal norms)
    what = U.STACK if channels == 3 else (U.DEV,)
    src = U.blocky_planes(h, w, 1, seed=3)
    want = U.expected(src, channels, R, what)
    with capi.Context(h, w, 1) as s, capi.Context(h, w, channels, p) as dst, capi.Context(h, w, channels, p) as control:
        s.set_image(src)
        for c in (dst, control):
            alone(c, trace=8)
            c.set_levelset(smooth_levelset(h, w))                   # before the planes arrive: kept, as cvh_set_image keeps it
        s.local_planes_to(dst, R, what)
        control.set_image(want)
        assert same_planes(dst.get_image(), want)
        assert np.array_equal(bits(dst.get_levelset()), bits(smooth_levelset(h, w)))
        assert dst.get_stop_condition() == control.get_stop_condition()
        for c in (dst, control):
            c.init_checkerboard()
        for x, y in zip(dst.get_means(), control.get_means()):
            assert np.array_equal(bits(x), bits(y))
        ra, rb = dst.run(5), control.run(5)
        assert ra[0] == rb[0] and bits(np.float64(ra[1])) == bits(np.float64(rb[1]))
        assert np.array_equal(bits(dst.get_trace(5)), bits(control.get_trace(5)))
        assert np.array_equal(bits(dst.get_levelset()), bits(control.get_levelset()))
        # iterations the destination has in flight are settled on its OLD planes, as cvh_set_image settles them
        for c in (dst, control):
            c.set_image(U.random_planes(h, w, channels, seed=9))
            c.set_levelset(smooth_levelset(h, w))
            c.enqueue_steps(8)
        s.local_planes_to(dst, R, what)                             # no sync in between
        control.set_image(want)
        sa, sb = dst.sync(), control.sync()
        assert sa[0] == sb[0] == 8 and bits(np.float64(sa[1])) == bits(np.float64(sb[1]))
        assert np.array_equal(bits(dst.get_levelset()), bits(control.get_levelset()))
        assert same_planes(dst.get_image(), want)


def test_source_is_only_read_and_its_iterations_stay_in_flight(capi):
    h, w = 64, 96
    p = capi.make_params(tol=2.0 ** -40)
    planes = U.blocky_planes(h, w, 3, seed=5)
    with capi.Context(h, w, 3, p) as src, capi.Context(h, w, 3, p) as twin, capi.Context(h, w, 3) as dst:
        for c in (src, twin):
            alone(c, trace=8)
            c.set_image(planes)
            c.set_levelset(smooth_levelset(h, w))
            c.enqueue_steps(4)
        src.local_planes_to(dst, 3, (U.DEV, U.MEAN, U.DEV))         # run 4, the call, run 4 is run 8
        for c in (src, twin):
            c.enqueue_steps(4)
        sa, sb = src.sync(), twin.sync()
        assert sa[0] == sb[0] == 8 and bits(np.float64(sa[1])) == bits(np.float64(sb[1]))
        assert np.array_equal(bits(src.get_levelset()), bits(twin.get_levelset()))
        assert np.array_equal(bits(src.get_trace(8)), bits(twin.get_trace(8)))
        assert same_planes(src.get_image(), planes)
        assert same_planes(dst.get_image(), U.expected(planes, 3, 3, (U.DEV, U.MEAN, U.DEV)))


def test_after_perona_malik_the_smoothed_planes_are_taken(capi):
    h, w = 64, 48
    planes = U.random_planes(h, w, 1, seed=2)
    with capi.Context(h, w, 1) as src, capi.Context(h, w, 1) as dst:
        src.set_image(planes)
        src.perona_malik(K=10.0, L=0.25, T=1.0)
        smoothed = src.get_image()
        assert not same_planes(smoothed, planes)
        src.local_planes_to(dst, 2, "dev")
        assert same_planes(dst.get_image(), U.expected(smoothed, 1, 2, (U.DEV,)))


def test_refusals_leave_the_planes_unchanged(capi):
    h, w = 17, 19
    planes = U.random_planes(h, w, 3)
    with capi.Context(h, w, 3) as a, capi.Context(h, w, 3) as b, capi.Context(h, w, 3) as empty, capi.Context(h, w, 1) as one, \
            capi.Context(h, w + 1, 1) as wide, capi.Context(h, w, 1) as dst:
        for c in (a, b):
            c.set_image(planes)
        for c in (one, dst):
            c.set_image(planes[:1])
        wide.set_image([np.zeros((h, w + 1), np.uint8)])
        L = capi.lib()
        I3 = ctypes.c_int * 3
        arr = lambda *cs: (ctypes.c_void_p * len(cs))(*[c._h for c in cs])

        def unchanged():
            return same_planes(a.get_image(), planes) and same_planes(b.get_image(), planes) and same_planes(one.get_image(), planes[:1]) \
                and same_planes(dst.get_image(), planes[:1]) and not wide.get_image()[0].any()

        refused = refusal_check(L, unchanged)                        # (whole=: the message byte for byte)

        ok = I3(U.DEV, U.MEAN, U.COPY)
        refused(L.cvh_local_planes(a._h, a._h, 1, ok), ERR_ARG, "cvh_local_planes", "pair 0")                      # src == dst
        refused(L.cvh_local_planes_batch(arr(a, b), arr(dst, dst), 2, (ctypes.c_int * 2)(1, 1), (ctypes.c_int * 6)()), ERR_ARG,
                "cvh_local_planes_batch", "pair 1", "pair 0")
        refused(L.cvh_local_planes_batch(arr(a, one), arr(dst, a), 2, (ctypes.c_int * 2)(1, 1), (ctypes.c_int * 6)()), ERR_ARG, "pair 1", "pair 0")
        refused(L.cvh_local_planes_batch(arr(a, b), arr(dst, wide), 2, (ctypes.c_int * 2)(1, 1), (ctypes.c_int * 6)()), ERR_ARG, "pair 1",
                f"{h} x {w}", whole="cvh_local_planes_batch: pair 1: the destination of a 17 x 19 source must be 17 x 19 too, got 17 x 20")
        for bad, whole in ((-1, "cvh_local_planes: pair 0: the radius must be 0 .. 127, got -1"),
                           (128, "cvh_local_planes: pair 0: the radius must be 0 .. 127, got 128"),
                           (1 << 20, "cvh_local_planes: pair 0: the radius must be 0 .. 127, got 1048576")):
            refused(L.cvh_local_planes(a._h, dst._h, bad, ok), ERR_ARG, "pair 0", "radius", whole=whole)
        refused(L.cvh_local_planes_batch(arr(a, b), arr(dst, one), 2, (ctypes.c_int * 2)(1, 200), (ctypes.c_int * 6)()), ERR_ARG, "pair 1", "radius",
                whole="cvh_local_planes_batch: pair 1: the radius must be 0 .. 127, got 200")
        for bad, whole in ((I3(3, 0, 0), "cvh_local_planes: pair 0: what[0] must be CVH_LOCAL_COPY (0), CVH_LOCAL_MEAN (1) or CVH_LOCAL_DEV (2), got 3"),
                           (I3(-1, 0, 0), "cvh_local_planes: pair 0: what[0] must be CVH_LOCAL_COPY (0), CVH_LOCAL_MEAN (1) or CVH_LOCAL_DEV (2), got -1")):
            refused(L.cvh_local_planes(a._h, dst._h, 1, bad), ERR_ARG, "pair 0", "what[0]", whole=whole)
        refused(L.cvh_local_planes(a._h, b._h, 1, I3(0, 1, 7)), ERR_ARG, "pair 0", "what[2]")
        refused(L.cvh_local_planes(a._h, dst._h, 1, None), ERR_ARG, "cvh_local_planes", "NULL", whole="cvh_local_planes: the list of codes (what) is NULL")
        refused(L.cvh_local_planes_batch(arr(a), arr(dst), 1, None, ok), ERR_ARG, "cvh_local_planes_batch", "NULL",
                whole="cvh_local_planes_batch: the list of radii is NULL")
        refused(L.cvh_local_planes_batch(arr(a), arr(dst), 0, (ctypes.c_int * 1)(1), ok), ERR_ARG, "cvh_local_planes_batch")
        refused(L.cvh_local_planes(empty._h, dst._h, 1, ok), ERR_STATE, "pair 0", "no image")
        refused(L.cvh_local_planes_batch(arr(a, empty), arr(dst, one), 2, (ctypes.c_int * 2)(1, 1), (ctypes.c_int * 6)()), ERR_STATE, "pair 1", "no image")
        # entries of `what` behind the destination's channels are ignored, and everything stays usable
        assert L.cvh_local_planes(a._h, dst._h, 2, I3(U.DEV, 99, -5)) == 0
        assert same_planes(dst.get_image(), U.expected(planes, 1, 2, (U.DEV,)))
        a.local_planes_to(empty, 1, "mean")                          # a destination needs no image of its own
        assert same_planes(empty.get_image(), U.expected(planes, 3, 1, (U.MEAN,) * 3))


def test_the_proposition_on_the_device(capi):
    """The local deviation row of the proposition (test_local_restatement.py) with the plane made and the run done on the device: the
    plane is the restatement's, the run ends at the oracle's iteration count -- the cap of 600 -- in the oracle's mask within the mask
    bar tests/test_gpu_parity.py states (IoU >= 0.999); the mask finds the disk (IoU >= 0.9, the CPU test's bar).  The distance of the two
    level sets is printed, not asserted: the run ends at the cap, not at a stop."""
    from oracle import cv_oracle as O
    u_c, steps_c, _ = U.oracle_proposition("dev")
    n = U.PROP_N
    with capi.Context(n, n, 1) as src, capi.Context(n, n, 1) as ctx:
        src.set_image([np.array(U.proposition_image())])
        src.local_planes_to(ctx, U.PROP_R, "dev")
        assert same_planes(ctx.get_image(), [U.proposition_plane("dev")])
        ctx.init_checkerboard()
        steps, _ = ctx.run(600)
        u_g, mask = ctx.get_levelset(), ctx.get_mask()
    err = float(np.abs(u_g - u_c).max() / np.abs(u_c).max())
    agree = U.iou(mask, O.mask(u_c))
    found = U.iou_either(U.proposition_truth(n), mask)
    print("steps", steps, steps_c, "rel err", err, "mask IoU with the oracle's", agree, "with the disk", found)
    assert steps == steps_c
    assert agree >= 0.999
    assert found >= 0.9
