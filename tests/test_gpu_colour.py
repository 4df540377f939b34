"""Colour spaces on the GPU (cvh_convert_colour*, cvh_luma_image*) against the numpy restatement of the header's definition
(colour_util).  The definition is in integers, so planes, stop conditions, means, traces and level sets are compared with == (on bit
patterns for doubles); only the proposition's run against the CPU oracle has bars, and they are the ones tests/test_gpu_parity.py states
for a run to its stop: the oracle's stop iteration, max|u_gpu - u_cpu| / max|u_cpu| <= 1e-6, mask IoU >= 0.999.  Not covered here: the
two CVH_ERR_ARG cases that no quick test can build -- contexts on different devices (needs two GPUs) and a plane of 2^32 pixels.
Run with -m gpu on an MI355X."""
import ctypes

import numpy as np
import pytest

import colour_util as U

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = 1, 3
ids = dict(ids=lambda s: f"{s[0]}x{s[1]}")


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def alone(ctx, **opts):
    """contexts compared in bits must not see each other in their automatic choices (tests/test_gpu_device_io.py, same_choices)"""
    ctx.set_option("co_resident", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def same_planes(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def same_state(a, b, start=True, steps=5):
    """a and b hold the same image: the stop condition, the means after the same start, a traced run and the level set behind it agree in
    bits (start = False: they already hold the same level set)"""
    if start:
        u0 = smooth_levelset(a.h, a.w)
        a.set_levelset(u0)
        b.set_levelset(u0)
    assert a.get_stop_condition() == b.get_stop_condition()
    for x, y in zip(a.get_means(), b.get_means()):
        assert np.array_equal(bits(x), bits(y))
    ra, rb = a.run(steps), b.run(steps)
    assert ra[0] == rb[0] and bits(np.float64(ra[1])) == bits(np.float64(rb[1]))
    assert np.array_equal(bits(a.get_trace(steps)), bits(b.get_trace(steps)))
    assert np.array_equal(bits(a.get_levelset()), bits(b.get_levelset()))


def smooth_levelset(h, w):
    ii, jj = np.mgrid[0:h, 0:w]
    return min(h, w) / 3.0 - np.hypot(ii - h / 2.0, jj - w / 2.0)


def launches():
    fn = ctypes.CDLL(__import__("chan_vese_amd").capi.LIB_PATH).cvh_debug_colour_launches
    fn.restype = ctypes.c_ulong
    return fn()


@pytest.mark.parametrize("order", U.ORDERS)
@pytest.mark.parametrize("space", U.SPACES)
@pytest.mark.parametrize("shape", U.SHAPES, **ids)
def test_convert_forward_and_inverse(capi, shape, space, order):
    h, w = shape
    with capi.Context(h, w, 3) as ctx:
        for kind in U.INPUTS:
            planes = U.planes_of(kind, h, w, order)
            ctx.set_image(planes)
            ctx.convert_colour(space, order)
            want = U.forward(planes, space, order)
            assert same_planes(ctx.get_image(), want), kind
            ctx.convert_colour(space, order, inverse=True)              # back, from what forward left
            assert same_planes(ctx.get_image(), U.inverse(want, space, order)), kind
            ctx.set_image(planes)                                       # and the inverse of bytes that were never converted
            ctx.convert_colour(space, order, inverse=True)
            assert same_planes(ctx.get_image(), U.inverse(planes, space, order)), kind
            if kind == "greys":
                assert same_planes(want, [planes[0], np.full((h, w), 128, np.uint8), np.full((h, w), 128, np.uint8)])


@pytest.mark.parametrize("shape", [(64, 48), (33, 257)], **ids)
def test_converted_context_equals_set_image_of_the_bytes(capi, shape):
    h, w = shape
    p = capi.make_params(tol=2.0 ** -40, lambda1=[0.25, 1, 0.5], lambda2=[0.5, 1, 0.75])   # (a power of two: equal stop conditions are equal norms)
    with capi.Context(h, w, 3, p) as ctx, capi.Context(h, w, 3, p) as control:
        for c in (ctx, control):
            alone(c, trace=8)
        for space, order, inv in (("ycrcb", "bgr", False), ("yuv", "rgb", False), ("ycrcb", "rgb", True)):
            planes = U.planes_of("random", h, w, order, seed=3)
            ctx.set_image(planes)
            ctx.convert_colour(space, order, inverse=inv)
            want = (U.inverse if inv else U.forward)(planes, space, order)
            assert same_planes(ctx.get_image(), want)
            control.set_image(want)
            same_state(ctx, control)


def test_convert_keeps_a_level_set_and_settles_iterations_in_flight(capi):
    h, w = 33, 257
    p = capi.make_params(tol=2.0 ** -40)
    planes = U.planes_of("random", h, w, "bgr", seed=1)
    want = U.forward(planes, "yuv", "bgr")
    with capi.Context(h, w, 3, p) as ctx, capi.Context(h, w, 3, p) as control:
        for c in (ctx, control):
            alone(c, trace=16)
            c.set_levelset(smooth_levelset(h, w))                       # a level set before any image
            c.set_image(planes)
        ctx.convert_colour("yuv", "bgr")
        control.set_image(want)
        assert np.array_equal(bits(ctx.get_levelset()), bits(smooth_levelset(h, w)))
        same_state(ctx, control, start=False)                           # the level set it held serves the new planes
        # iterations in flight: settled on the OLD planes, as cvh_set_image settles them
        for c in (ctx, control):
            c.set_image(planes)
            c.set_levelset(smooth_levelset(h, w))
            c.enqueue_steps(8)
        ctx.convert_colour("yuv", "bgr")                                # no sync in between
        control.set_image(want)
        sa, sb = ctx.sync(), control.sync()
        assert sa[0] == sb[0] == 8 and bits(np.float64(sa[1])) == bits(np.float64(sb[1])) and sa[2] == sb[2]
        assert np.array_equal(bits(ctx.get_levelset()), bits(control.get_levelset()))
        assert same_planes(ctx.get_image(), want)
        same_state(ctx, control, start=False)


def test_convert_after_perona_malik_takes_the_smoothed_planes(capi):
    h, w = 64, 48
    planes = U.planes_of("random", h, w, "rgb", seed=2)
    with capi.Context(h, w, 3) as ctx:
        ctx.set_image(planes)
        ctx.perona_malik(K=10.0, L=0.25, T=1.0)
        smoothed = ctx.get_image()
        assert not same_planes(smoothed, planes)
        ctx.convert_colour("ycrcb", "rgb")
        assert same_planes(ctx.get_image(), U.forward(smoothed, "ycrcb", "rgb"))


@pytest.mark.parametrize("order", U.ORDERS)
@pytest.mark.parametrize("shape", U.SHAPES, **ids)
def test_luma(capi, shape, order):
    h, w = shape
    p = capi.make_params(tol=2.0 ** -40)
    with capi.Context(h, w, 3, p) as src, capi.Context(h, w, 3, p) as twin, capi.Context(h, w, 1, p) as dst, capi.Context(h, w, 1, p) as control:
        for c in (src, twin, dst, control):
            alone(c, trace=8)
        for c in (dst, control):
            c.set_levelset(smooth_levelset(h, w))                       # before the plane arrives: kept, as cvh_set_image keeps it
        for kind in U.INPUTS:
            planes = U.planes_of(kind, h, w, order)
            src.set_image(planes)
            src.luma_to(dst, order)
            want = U.luma(planes, order)
            assert same_planes(dst.get_image(), [want]), kind
            control.set_image([want])
            assert dst.get_stop_condition() == control.get_stop_condition(), kind       # one channel: sum p^2, an exact integer
            assert same_planes(src.get_image(), planes), kind
        assert np.array_equal(bits(dst.get_levelset()), bits(smooth_levelset(h, w)))
        planes = U.planes_of("random", h, w, order)
        src.set_image(planes)
        src.luma_to(dst, order)
        control.set_image([U.luma(planes, order)])
        same_state(dst, control)
        # the source is only read, its iterations stay in flight across the call: run 4, luma, run 4 is run 8
        twin.set_image(planes)
        for c in (src, twin):
            c.set_levelset(smooth_levelset(h, w))
            c.enqueue_steps(4)
        src.luma_to(dst, order)
        for c in (src, twin):
            c.enqueue_steps(4)
        sa, sb = src.sync(), twin.sync()
        assert sa[0] == sb[0] == 8 and bits(np.float64(sa[1])) == bits(np.float64(sb[1]))
        assert np.array_equal(bits(src.get_levelset()), bits(twin.get_levelset()))
        assert np.array_equal(bits(src.get_trace(8)), bits(twin.get_trace(8)))
        assert same_planes(src.get_image(), planes) and same_planes(dst.get_image(), [U.luma(planes, order)])


def test_batches_equal_the_single_calls(capi):
    p = capi.make_params(tol=1.0)
    make = lambda ch: [capi.Context(*s, ch, p) for s in U.SHAPES]
    batch, single, dst_b, dst_s = make(3), make(3), make(1), make(1)
    try:
        for c in batch + single:
            alone(c, trace=8)
        for c in batch + single + dst_b + dst_s:
            c.set_levelset(smooth_levelset(c.h, c.w))                   # (the stop condition is asked of a context with a level set)
        imgs = [U.planes_of("random", *s, "bgr", seed=5) for s in U.SHAPES]
        for group in (batch, single):
            for c, img in zip(group, imgs):
                c.set_image(img)
        n0 = launches()
        capi.luma_image_batch(batch, dst_b, "bgr")
        assert launches() == n0 + 1                     # five pairs of five shapes, ONE launch
        for s, d in zip(single, dst_s):
            s.luma_to(d, "bgr")
        for b, s, img in zip(dst_b, dst_s, imgs):
            assert same_planes(b.get_image(), s.get_image()) and same_planes(b.get_image(), [U.luma(img, "bgr")])
            assert b.get_stop_condition() == s.get_stop_condition()
        for inv in (False, True):
            n0 = launches()
            capi.convert_colour_batch(batch, "ycrcb", "bgr", inverse=inv)
            assert launches() == n0 + 1                 # five members, ONE launch
            for s in single:
                s.convert_colour("ycrcb", "bgr", inverse=inv)
            imgs = [(U.inverse if inv else U.forward)(img, "ycrcb", "bgr") for img in imgs]
            for b, s, img in zip(batch, single, imgs):
                assert same_planes(b.get_image(), s.get_image()) and same_planes(b.get_image(), img)
                assert b.get_stop_condition() == s.get_stop_condition()
        for b, s in zip(batch, single):
            same_state(b, s)
    finally:
        for c in batch + single + dst_b + dst_s:
            c.close()


def test_error_paths_leave_the_members_usable(capi):
    h, w = 17, 19
    planes = U.planes_of("random", h, w)
    with capi.Context(h, w, 3) as a, capi.Context(h, w, 3) as b, capi.Context(h, w, 3) as empty, capi.Context(h, w, 1) as one, \
            capi.Context(h, w + 1, 1) as wide, capi.Context(h, w, 1) as dst:
        for c in (a, b):
            c.set_image(planes)
        one.set_image(planes[:1])
        L = capi.lib()

        def refused(call, code, *words):
            with pytest.raises(capi.CvhError) as e:
                call()
            assert e.value.code == code
            msg = L.cvh_last_error(None).decode()
            assert all(word in msg for word in words), msg
            assert same_planes(a.get_image(), planes) and same_planes(b.get_image(), planes) and same_planes(one.get_image(), planes[:1])

        refused(lambda: capi.convert_colour_batch([a, b, a], "yuv"), ERR_ARG, "cvh_convert_colour_batch", "member 2", "member 0")
        refused(lambda: capi.convert_colour_batch([a, one], "yuv"), ERR_ARG, "member 1", "channel")
        refused(lambda: one.convert_colour("ycrcb"), ERR_ARG, "cvh_convert_colour", "member 0")
        refused(lambda: capi.convert_colour_batch([a, empty], "yuv"), ERR_STATE, "member 1", "no image")
        for bad in ((0, 0, 0), (3, 0, 0), (1, 2, 0), (1, -1, 0), (1, 0, 2), (1, 0, -1)):
            assert L.cvh_convert_colour(a._h, *bad) == ERR_ARG
        assert L.cvh_luma_image(a._h, dst._h, 2) == ERR_ARG
        refused(lambda: capi.luma_image_batch([a, b], [dst, wide]), ERR_ARG, "cvh_luma_image_batch", "pair 1", f"{h} x {w}")
        refused(lambda: capi.luma_image_batch([a, b], [dst, dst]), ERR_ARG, "pair 1", "pair 0")
        refused(lambda: a.luma_to(a), ERR_ARG, "cvh_luma_image", "pair 0")
        refused(lambda: one.luma_to(dst), ERR_ARG, "pair 0", "source")
        refused(lambda: a.luma_to(b), ERR_ARG, "pair 0", "destination")
        refused(lambda: capi.luma_image_batch([a, empty], [dst, one]), ERR_STATE, "pair 1", "no image")
        # all of them stay usable
        capi.convert_colour_batch([a, b], "yuv")
        assert same_planes(a.get_image(), U.forward(planes, "yuv", "bgr")) and same_planes(b.get_image(), a.get_image())
        b.luma_to(one)
        assert same_planes(one.get_image(), [U.luma(b.get_image(), "bgr")])


def test_every_colour_once(capi):
    """4096 x 4096 x 3 holding every one of the 2^24 colours once, forward in both spaces: the one test whose size is the point (two
    uploads, two conversions; the planes also pass the 2048-workgroup cap of the grid, so every lane makes several trips)."""
    planes = U.every_colour_planes()
    with capi.Context(4096, 4096, 3) as ctx:
        for space in U.SPACES:
            ctx.set_image(planes)
            ctx.convert_colour(space, "rgb")
            assert same_planes(ctx.get_image(), U.forward(planes, space, "rgb")), space


def test_the_proposition_on_the_device(capi):
    """The (Y, Cr, Cb), lambda = (0, 1, 1) row of the proposition (test_colour_api.py) with the conversion and the run on the device:
    the planes are the restatement's, the run stops at the oracle's iteration and ends in the oracle's level set and mask within the
    bars tests/test_gpu_parity.py states for a run to its stop; the mask finds the disk (IoU >= 0.85, the CPU test's bar)."""
    from oracle import cv_oracle as O
    row = 2
    space, lam = U.PROP_ROWS[row]
    u_c, steps_c, _ = U.oracle_proposition(row)
    n = U.PROP_N
    with capi.Context(n, n, 3, capi.make_params(lambda1=lam, lambda2=lam)) as ctx:
        ctx.set_image(U.proposition_image())
        ctx.convert_colour(space, "rgb")
        assert same_planes(ctx.get_image(), U.proposition_planes(space))
        ctx.init_checkerboard()
        steps, _ = ctx.run(600)
        u_g, mask = ctx.get_levelset(), ctx.get_mask()
    err = float(np.abs(u_g - u_c).max() / np.abs(u_c).max())
    agree = U.iou(mask, O.mask(u_c))
    found = U.iou_either(U.proposition_truth(n), mask)
    print("steps", steps, steps_c, "rel err", err, "mask IoU with the oracle's", agree, "with the disk", found)
    assert steps == steps_c
    assert err <= 1e-6
    assert agree >= 0.999
    assert found >= 0.85


def test_cli_colorspace_runs_the_proposition(capi, tmp_path):
    """bin/chan_vese --colorspace ycrcb --lambda1 0 1 1 --lambda2 0 1 1 on the proposition's image as a PPM: the loader's B, G, R planes,
    converted on the device, give the oracle's run of the converted planes -- its stop iteration and, within the mask bar of
    tests/test_gpu_parity.py (IoU >= 0.999), its mask; without --colorspace the same command does not find the disk (the CPU test's
    bar for R, G, B: IoU <= 0.5)."""
    import os
    import subprocess
    from oracle import cv_oracle as O
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    n = U.PROP_N
    img = tmp_path / "prop.ppm"
    with open(img, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (n, n) + np.ascontiguousarray(np.stack(U.proposition_image(), axis=-1)).tobytes())
    masks = {}
    for name, extra in (("ycrcb", ["--colorspace", "ycrcb"]), ("rgb", [])):
        out = tmp_path / f"{name}.pgm"
        r = subprocess.run([os.path.join(root, "bin", "chan_vese"), "-i", str(img), "--lambda1", "0", "1", "1", "--lambda2", "0", "1", "1",
                            "-N", "600", "--dump-mask", str(out), "--verbose", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        raw = open(out, "rb").read()
        masks[name] = (np.frombuffer(raw[-n * n:], dtype=np.uint8).reshape(n, n) != 0, r.stderr)
    u_c, steps_c, _ = U.oracle_proposition(2)
    assert f"chan_vese: {steps_c} iterations" in masks["ycrcb"][1]
    assert U.iou(masks["ycrcb"][0], O.mask(u_c)) >= 0.999
    assert U.iou_either(U.proposition_truth(n), masks["ycrcb"][0]) >= 0.85
    assert U.iou_either(U.proposition_truth(n), masks["rgb"][0]) <= 0.5
