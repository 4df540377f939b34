"""Rank planes on the GPU (cvh_rank_planes, cvh_rank_planes_batch) against the fast restatement of the header's definition
(rank_util).  The definition is in integers, so planes, stop conditions, means, traces and level sets are compared with == (on bit
patterns for doubles); only the propositions' runs against the CPU oracle have a bar, the mask bar tests/test_gpu_parity.py states.
Not covered here: the two CVH_ERR_ARG cases that no quick test can build -- contexts on different devices (needs two GPUs) and a plane
of 2^32 pixels -- and a second trip of the column passes, which takes a plane of more than 2^25 pixels (the row pass and the median make
their second trips in the large case).  Run with -m gpu on an MI355X."""
import ctypes

import numpy as np
import pytest

import rank_util as U
from window_util import alone, bits, device_capi, launch_sets, refusal_check, same_planes, smooth_levelset

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = 1, 3
SEPARABLE = (U.MIN, U.MAX, U.OPEN, U.CLOSE, U.TOPHAT, U.BOTHAT)


@pytest.fixture(scope="module")
def capi():
    return device_capi()


@pytest.mark.parametrize("case", U.CASES, ids=lambda c: "%dx%d-R%d-%s" % c)
def test_separable_codes_equal_the_restatement(capi, case):
    """every separable code 1 -> 1, then triples that share chains, 1 -> 3 and 3 -> 3, and 3 -> 1: every byte"""
    h, w, R, kind = case
    src1, src3 = U.case_planes(kind, h, w, 1, seed=1), U.case_planes(kind, h, w, 3, seed=2)
    with capi.Context(h, w, 1) as s1, capi.Context(h, w, 3) as s3, capi.Context(h, w, 1) as d1, capi.Context(h, w, 3) as d3:
        s1.set_image(src1)
        s3.set_image(src3)
        for code in SEPARABLE:
            s1.rank_planes_to(d1, R, (code,))
            assert same_planes(d1.get_image(), U.expected(src1, 1, R, (code,))), code
        for what in ((U.OPEN, U.TOPHAT, U.COPY), (U.MIN, U.OPEN, U.MAX), (U.BOTHAT, U.MAX, U.CLOSE)):
            s1.rank_planes_to(d3, R, what)
            assert same_planes(d3.get_image(), U.expected(src1, 3, R, what)), what
        for what in ((U.TOPHAT, U.MIN, U.CLOSE), (U.MAX, U.COPY, U.OPEN)):
            s3.rank_planes_to(d3, R, what)
            assert same_planes(d3.get_image(), U.expected(src3, 3, R, what)), what
        s3.rank_planes_to(d1, R, "close")                           # 3 -> 1: plane 0 of the source
        assert same_planes(d1.get_image(), U.expected(src3, 1, R, (U.CLOSE,)))
        assert same_planes(s1.get_image(), src1) and same_planes(s3.get_image(), src3)


@pytest.mark.parametrize("case", U.MEDIAN_CASES, ids=lambda c: "%dx%d-R%d-%s" % c)
def test_median_equals_the_restatement(capi, case):
    h, w, R, kind = case
    src1, src3 = U.case_planes(kind, h, w, 1, seed=3), U.case_planes(kind, h, w, 3, seed=4)
    with capi.Context(h, w, 1) as s1, capi.Context(h, w, 3) as s3, capi.Context(h, w, 1) as d1, capi.Context(h, w, 3) as d3:
        s1.set_image(src1)
        s3.set_image(src3)
        s1.rank_planes_to(d1, R, "median")
        assert same_planes(d1.get_image(), U.expected(src1, 1, R, (U.MEDIAN,)))
        s3.rank_planes_to(d3, R, (U.MEDIAN, U.COPY, U.MEDIAN))
        assert same_planes(d3.get_image(), U.expected(src3, 3, R, (U.MEDIAN, U.COPY, U.MEDIAN)))
        s1.rank_planes_to(d3, R, (U.MEDIAN, U.TOPHAT, U.MEDIAN))   # one median plane, written twice
        assert same_planes(d3.get_image(), U.expected(src1, 3, R, (U.MEDIAN, U.TOPHAT, U.MEDIAN)))
        assert same_planes(s1.get_image(), src1) and same_planes(s3.get_image(), src3)


def test_large_plane_once(capi):
    h, w, R, kind = U.LARGE
    src = U.planes_of(kind, h, w, 1, seed=4)
    what = (U.MEDIAN, U.OPEN, U.TOPHAT)
    with capi.Context(h, w, 1) as s, capi.Context(h, w, 3) as d:
        s.set_image(src)
        s.rank_planes_to(d, R, what)
        assert same_planes(d.get_image(), U.expected(src, 3, R, what))


def test_copies_alone_launch_only_the_writer_and_radius_zero(capi):
    h, w = 33, 67
    src = U.random_planes(h, w, 3, seed=6)
    with capi.Context(h, w, 3) as s, capi.Context(h, w, 3) as d:
        s.set_image(src)
        s.rank_planes_to(d, 5, (U.COPY, U.COPY, U.COPY))
        assert same_planes(d.get_image(), src)
        s.rank_planes_to(d, 0, (U.MEDIAN, U.TOPHAT, U.CLOSE))
        assert same_planes(d.get_image(), [src[0], np.zeros((h, w), np.uint8), src[2]])


def test_mixed_batch_equals_the_single_calls(capi):
    """1 -> 1, 1 -> 3, 3 -> 3 and 3 -> 1 pairs of four shapes, radii and codes, median pairs among the others, in ONE call"""
    pairs = [((33, 67), 1, 1, 5, (U.TOPHAT,)), ((U.BAND + 1, U.STRIP + 1), 1, 3, 2, (U.COPY, U.OPEN, U.MEDIAN)),
             ((40, 50), 3, 3, 127, (U.MAX, U.COPY, U.BOTHAT)), ((17, 300), 3, 1, 7, (U.MEDIAN,)), ((9, 11), 1, 1, 0, (U.MIN,))]
    srcs = [capi.Context(*s, cs) for s, cs, _, _, _ in pairs]
    dst_b = [capi.Context(*s, cd) for s, _, cd, _, _ in pairs]
    dst_s = [capi.Context(*s, cd) for s, _, cd, _, _ in pairs]
    try:
        imgs = [U.blocky_planes(*s, cs, seed=i) for i, (s, cs, _, _, _) in enumerate(pairs)]
        for c, img in zip(srcs, imgs):
            c.set_image(img)
        for c in dst_b + dst_s:
            c.set_levelset(smooth_levelset(c.h, c.w))               # (the stop condition is asked of a context with a level set)
        n0 = launch_sets("rank")
        capi.rank_planes_batch(srcs, dst_b, [p[3] for p in pairs], [p[4] for p in pairs])
        assert launch_sets("rank") == n0 + 1                              # five pairs, ONE set of launches
        for s, d, p in zip(srcs, dst_s, pairs):
            s.rank_planes_to(d, p[3], p[4])
        for b, s, img, p in zip(dst_b, dst_s, imgs, pairs):
            assert same_planes(b.get_image(), s.get_image()) and same_planes(b.get_image(), U.expected(img, p[2], p[3], p[4] + (0, 0)))
            assert b.get_stop_condition() == s.get_stop_condition()
        # a scalar radius and one name go to every pair; then a batch of COPY alone
        capi.rank_planes_batch(srcs[:2], dst_b[:2], 3, "bothat")
        for b, img, p in zip(dst_b[:2], imgs[:2], pairs[:2]):
            assert same_planes(b.get_image(), U.expected(img, p[2], 3, (U.BOTHAT,) * 3))
        capi.rank_planes_batch(srcs[:3], dst_b[:3], 9, (U.COPY, U.COPY, U.COPY))
        for b, img, p in zip(dst_b[:3], imgs[:3], pairs[:3]):
            assert same_planes(b.get_image(), U.expected(img, p[2], 9, (U.COPY,) * 3))
    finally:
        for c in srcs + dst_b + dst_s:
            c.close()


@pytest.mark.parametrize("channels", [1, 3])
def test_destination_equals_set_image_of_the_bytes(capi, channels):
    h, w, R = 33, 257, 4
    p = capi.make_params(tol=2.0 ** -40, lambda1=[0.25, 1, 0.5], lambda2=[0.5, 1, 0.75])   # (a power of two: equal stop conditions are equal norms)
    what = (U.MEDIAN, U.OPEN, U.TOPHAT) if channels == 3 else (U.CLOSE,)
    src = U.blocky_planes(h, w, 1, seed=3)
    want = U.expected(src, channels, R, what)
    with capi.Context(h, w, 1) as s, capi.Context(h, w, channels, p) as dst, capi.Context(h, w, channels, p) as control:
        s.set_image(src)
        for c in (dst, control):
            alone(c, trace=8)
            c.set_levelset(smooth_levelset(h, w))                   # before the planes arrive: kept, as cvh_set_image keeps it
        s.rank_planes_to(dst, R, what)
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
        s.rank_planes_to(dst, R, what)                              # no sync in between
        control.set_image(want)
        sa, sb = dst.sync(), control.sync()
        assert sa[0] == sb[0] == 8 and bits(np.float64(sa[1])) == bits(np.float64(sb[1]))
        assert np.array_equal(bits(dst.get_levelset()), bits(control.get_levelset()))
        assert same_planes(dst.get_image(), want)


def test_source_is_only_read_and_its_iterations_stay_in_flight(capi):
    h, w = 64, 96
    p = capi.make_params(tol=2.0 ** -40)
    planes = U.blocky_planes(h, w, 3, seed=5)
    what = (U.MEDIAN, U.TOPHAT, U.MIN)
    with capi.Context(h, w, 3, p) as src, capi.Context(h, w, 3, p) as twin, capi.Context(h, w, 3) as dst:
        for c in (src, twin):
            alone(c, trace=8)
            c.set_image(planes)
            c.set_levelset(smooth_levelset(h, w))
            c.enqueue_steps(4)
        src.rank_planes_to(dst, 3, what)                            # run 4, the call, run 4 is run 8
        for c in (src, twin):
            c.enqueue_steps(4)
        sa, sb = src.sync(), twin.sync()
        assert sa[0] == sb[0] == 8 and bits(np.float64(sa[1])) == bits(np.float64(sb[1]))
        assert np.array_equal(bits(src.get_levelset()), bits(twin.get_levelset()))
        assert np.array_equal(bits(src.get_trace(8)), bits(twin.get_trace(8)))
        assert same_planes(src.get_image(), planes)
        assert same_planes(dst.get_image(), U.expected(planes, 3, 3, what))


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

        ok = I3(U.OPEN, U.MAX, U.COPY)
        two = lambda x, y: (ctypes.c_int * 2)(x, y)
        refused(L.cvh_rank_planes(a._h, a._h, 1, ok), ERR_ARG, "cvh_rank_planes", "pair 0")                      # src == dst
        refused(L.cvh_rank_planes_batch(arr(a, b), arr(dst, dst), 2, two(1, 1), (ctypes.c_int * 6)()), ERR_ARG, "cvh_rank_planes_batch", "pair 1", "pair 0")
        refused(L.cvh_rank_planes_batch(arr(a, one), arr(dst, a), 2, two(1, 1), (ctypes.c_int * 6)()), ERR_ARG, "pair 1", "pair 0")
        refused(L.cvh_rank_planes_batch(arr(a, b), arr(dst, wide), 2, two(1, 1), (ctypes.c_int * 6)()), ERR_ARG, "pair 1", f"{h} x {w}",
                whole="cvh_rank_planes_batch: pair 1: the destination of a 17 x 19 source must be 17 x 19 too, got 17 x 20")
        for bad, whole in ((-1, "cvh_rank_planes: pair 0: the radius must be 0 .. 127, got -1"),
                           (128, "cvh_rank_planes: pair 0: the radius must be 0 .. 127, got 128"),
                           (1 << 20, "cvh_rank_planes: pair 0: the radius must be 0 .. 127, got 1048576")):
            refused(L.cvh_rank_planes(a._h, dst._h, bad, ok), ERR_ARG, "pair 0", "radius", whole=whole)
        refused(L.cvh_rank_planes_batch(arr(a, b), arr(dst, one), 2, two(1, 200), (ctypes.c_int * 6)()), ERR_ARG, "pair 1", "radius",
                whole="cvh_rank_planes_batch: pair 1: the radius must be 0 .. 127, got 200")
        for bad, whole in ((I3(8, 0, 0), "cvh_rank_planes: pair 0: what[0] must be one of CVH_RANK_COPY (0) .. CVH_RANK_BOTHAT (7), got 8"),
                           (I3(-1, 0, 0), "cvh_rank_planes: pair 0: what[0] must be one of CVH_RANK_COPY (0) .. CVH_RANK_BOTHAT (7), got -1")):
            refused(L.cvh_rank_planes(a._h, dst._h, 1, bad), ERR_ARG, "pair 0", "what[0]", whole=whole)
        refused(L.cvh_rank_planes(a._h, b._h, 1, I3(0, 1, 9)), ERR_ARG, "pair 0", "what[2]")
        refused(L.cvh_rank_planes(a._h, dst._h, 8, I3(U.MEDIAN, 0, 0)), ERR_ARG, "pair 0", "median", "radius",      # the median's limit
                whole="cvh_rank_planes: pair 0: the radius of a median (what[0]) must be 0 .. 7, got 8")
        refused(L.cvh_rank_planes(a._h, b._h, 127, I3(U.MAX, U.OPEN, U.MEDIAN)), ERR_ARG, "pair 0", "median", "what[2]",
                whole="cvh_rank_planes: pair 0: the radius of a median (what[2]) must be 0 .. 7, got 127")
        refused(L.cvh_rank_planes_batch(arr(a, b), arr(dst, one), 2, two(7, 8), (ctypes.c_int * 6)(3, 0, 0, 3, 0, 0)), ERR_ARG, "pair 1", "median",
                whole="cvh_rank_planes_batch: pair 1: the radius of a median (what[0]) must be 0 .. 7, got 8")
        refused(L.cvh_rank_planes(a._h, dst._h, 1, None), ERR_ARG, "cvh_rank_planes", "NULL", whole="cvh_rank_planes: the list of codes (what) is NULL")
        refused(L.cvh_rank_planes_batch(arr(a), arr(dst), 1, None, ok), ERR_ARG, "cvh_rank_planes_batch", "NULL",
                whole="cvh_rank_planes_batch: the list of radii is NULL")
        refused(L.cvh_rank_planes_batch(arr(a), arr(dst), 0, (ctypes.c_int * 1)(1), ok), ERR_ARG, "cvh_rank_planes_batch")
        refused(L.cvh_rank_planes(empty._h, dst._h, 1, ok), ERR_STATE, "pair 0", "no image")
        refused(L.cvh_rank_planes_batch(arr(a, empty), arr(dst, one), 2, two(1, 1), (ctypes.c_int * 6)()), ERR_STATE, "pair 1", "no image")
        # entries of `what` behind the destination's channels are ignored -- a median there does not bind the radius --, and everything stays usable
        assert L.cvh_rank_planes(a._h, dst._h, 20, I3(U.TOPHAT, U.MEDIAN, -5)) == 0
        assert same_planes(dst.get_image(), U.expected(planes, 1, 20, (U.TOPHAT,)))
        a.rank_planes_to(empty, 1, "median")                         # a destination needs no image of its own
        assert same_planes(empty.get_image(), U.expected(planes, 3, 1, (U.MEDIAN,) * 3))


@pytest.mark.parametrize("name", ["salt median R=2", "ramp tophat R=10"])
def test_the_propositions_on_the_device(capi, name):
    """A row of the propositions (test_rank_restatement.py) with the plane made and the run done on the device: the plane is the
    restatement's, the run takes the oracle's iteration count and ends in the oracle's mask within the mask bar tests/test_gpu_parity.py
    states (IoU >= 0.999).  The distance of the two level sets is printed, not asserted."""
    from oracle import cv_oracle as O
    u_c, steps_c, _ = U.oracle_proposition(name)
    image, code, R, truth = U.PROPOSITIONS[name]
    n = U.PROP_N
    with capi.Context(n, n, 1) as src, capi.Context(n, n, 1) as ctx:
        src.set_image([np.array(image())])
        src.rank_planes_to(ctx, R, (code,))
        assert same_planes(ctx.get_image(), [U.proposition_plane(name)])
        ctx.init_checkerboard()
        steps, _ = ctx.run(600)
        u_g, mask = ctx.get_levelset(), ctx.get_mask()
    err = float(np.abs(u_g - u_c).max() / np.abs(u_c).max())
    agree = U.iou(mask, O.mask(u_c))
    print(name, "steps", steps, steps_c, "rel err", err, "mask IoU with the oracle's", agree, "with the truth", U.iou_either(truth(), mask))
    assert steps == steps_c
    assert agree >= 0.999
