"""Colour spaces without a GPU: the facts of the header's integer definition over all 2^24 colours (colour_util's restatement), the
exported symbols, the argument errors that need no device, capi's and the Segmenter's validation -- and the proposition itself on the CPU
oracle: under an illumination ramp a run on R, G, B segments the ramp, a run on (Y, Cr, Cb) with the luma weighted 0 finds the disk."""
import ctypes
import os

import numpy as np
import pytest

import colour_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvh_convert_colour", "cvh_convert_colour_batch", "cvh_luma_image", "cvh_luma_image_batch"]


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    return m


def test_facts_of_the_definition_over_all_colours():
    r, g, b = U.all_colours()
    y, cr, cb = U.raw_forward(r, g, b, "ycrcb")
    y2, u, v = U.raw_forward(r, g, b, "yuv")
    assert np.array_equal(y, y2)
    assert (y.min(), y.max()) == (0, 255)
    assert (cr.min(), cr.max()) == (0, 256)                                    # one value, 256, clamps
    assert (cb.min(), cb.max()) == (1, 255)
    assert (v.min(), v.max()) == (-29, 285)
    assert (u.min(), u.max()) == (17, 239)
    grey = r == g
    grey &= g == b
    assert grey.sum() == 256
    for space, (p1, p2) in (("ycrcb", (cr, cb)), ("yuv", (u, v))):
        assert np.array_equal(y[grey], r[grey]) and (p1[grey] == 128).all() and (p2[grey] == 128).all()
        back = U.inverse_rgb(y, np.clip(p1, 0, 255), np.clip(p2, 0, 255), space)
        for q, src in zip(back, (r, g, b)):
            assert np.array_equal(q[grey], src[grey])                          # a grey pixel comes back exactly
        err = [int(np.abs(q - src).max()) for q, src in zip(back, (r, g, b))]
        assert err == ([1, 1, 1] if space == "ycrcb" else [34, 17, 1])
        if space == "yuv":                                                     # the large errors sit where V clamped, nowhere else
            fits = (p2 >= 0) & (p2 <= 255)
            assert all(int(np.abs(q - src)[fits].max()) <= 1 for q, src in zip(back, (r, g, b)))


def test_restatement_forms_agree():
    """forward / inverse / luma on planes in either order are raw_forward / inverse_rgb on (R, G, B); the clampers reach the extremes"""
    for order in U.ORDERS:
        planes = U.planes_of("random", 17, 19, order)
        r, g, b = (planes[2], planes[1], planes[0]) if order == "bgr" else planes
        assert np.array_equal(U.luma(planes, order), U.luma_rgb(r, g, b).astype(np.uint8))
        for space in U.SPACES:
            f = U.forward(planes, space, order)
            assert all(p.dtype == np.uint8 and p.shape == (17, 19) for p in f)
            assert np.array_equal(f[0], U.luma(planes, order))
            assert np.array_equal(f[1], np.clip(U.raw_forward(r, g, b, space)[1], 0, 255))
            inv = U.inverse(f, space, order)
            rr, gg, bb = U.inverse_rgb(*f, space)
            want = [bb, gg, rr] if order == "bgr" else [rr, gg, bb]
            assert all(np.array_equal(a, w) for a, w in zip(inv, want))
    cl = U.planes_of("clampers", 16, 16, "rgb")
    assert U.raw_forward(*cl, "ycrcb")[1].min() == 0 and U.raw_forward(*cl, "ycrcb")[1].max() == 256
    assert U.raw_forward(*cl, "yuv")[2].min() == -29 and U.raw_forward(*cl, "yuv")[2].max() == 285
    assert U.raw_forward(*cl, "ycrcb")[2].min() == 1 and U.raw_forward(*cl, "yuv")[1].max() == 239
    assert len(set(U.SHAPES)) == 5 and U.SHAPES[-1][0] * U.SHAPES[-1][1] == U.BLOCK_PIXELS + U.PIECE


def test_new_symbols_are_exported(capi):
    header = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name) and f"int {name}(" in header
    assert "Colour spaces" in header
    for text in ("#define CVH_ORDER_BGR 0", "#define CVH_ORDER_RGB 1", "#define CVH_COLOUR_YCRCB 1", "#define CVH_COLOUR_YUV 2"):
        assert text in header
    assert capi.ORDERS == {"bgr": 0, "rgb": 1} and capi.COLOUR_SPACES == {"ycrcb": 1, "yuv": 2}
    for name in ("convert_colour_batch", "luma_image_batch"):
        assert callable(getattr(capi, name))
    assert callable(capi.Context.convert_colour) and callable(capi.Context.luma_to)
    L = ctypes.CDLL(capi.LIB_PATH)
    assert L.cvh_debug_colour_block_pixels() == U.BLOCK_PIXELS      # the shapes' "one workgroup + one piece" is the kernel's
    L.cvh_debug_colour_launches.restype = ctypes.c_ulong
    assert L.cvh_debug_colour_launches() >= 0


def test_argument_errors_without_a_device(capi):
    L = capi.lib()
    err = lambda: L.cvh_last_error(None).decode()
    assert L.cvh_convert_colour_batch(None, 1, 1, 0, 0) == 1 and "cvh_convert_colour_batch" in err()
    empty = (ctypes.c_void_p * 1)()
    assert L.cvh_convert_colour_batch(empty, 0, 1, 0, 0) == 1 and "cvh_convert_colour_batch" in err()
    assert L.cvh_convert_colour_batch(empty, 1, 1, 0, 0) == 1 and "member 0" in err()
    assert L.cvh_convert_colour(None, 1, 0, 0) == 1 and "cvh_convert_colour" in err() and "member 0" in err()
    assert L.cvh_luma_image_batch(None, None, 1, 0) == 1 and "cvh_luma_image_batch" in err()
    assert L.cvh_luma_image_batch(empty, empty, 0, 0) == 1 and "cvh_luma_image_batch" in err()
    assert L.cvh_luma_image_batch(empty, empty, 1, 0) == 1 and "pair 0" in err()
    assert L.cvh_luma_image(None, None, 0) == 1 and "cvh_luma_image" in err() and "pair 0" in err()


def test_capi_validates_strings_before_the_library(capi):
    assert capi.colour_space_code("ycrcb") == 1 and capi.colour_space_code("YUV") == 2
    assert capi.order_code("bgr") == 0 and capi.order_code("RGB") == 1
    for bad in ("lab", "", None, 1, "rgb"):
        with pytest.raises(ValueError, match="colour space"):
            capi.colour_space_code(bad)
        with pytest.raises(ValueError, match="colour space"):
            capi.convert_colour_batch([], bad)                # refused before the (empty) list reaches the library
    for bad in ("gbr", "", None, 0, "yuv"):
        with pytest.raises(ValueError, match="plane order"):
            capi.order_code(bad)
        with pytest.raises(ValueError, match="plane order"):
            capi.convert_colour_batch([], "yuv", bad)
        with pytest.raises(ValueError, match="plane order"):
            capi.luma_image_batch([], [], bad)
    with pytest.raises(ValueError, match="pair up"):
        capi.luma_image_batch([], [None])
    ctx = object.__new__(capi.Context)                        # no context is created: the strings are checked first
    with pytest.raises(ValueError, match="colour space"):
        capi.Context.convert_colour(ctx, "hsv")
    with pytest.raises(ValueError, match="plane order"):
        capi.Context.luma_to(ctx, ctx, "xyz")


def test_segmenter_validates_colour_without_a_gpu(capi):
    pytest.importorskip("torch")
    from chan_vese_amd import torch_io
    assert torch_io.check_colour(None, "rgb", 1) == (None, "rgb")
    assert torch_io.check_colour("YCrCb", "BGR", 3) == ("ycrcb", "bgr")
    with pytest.raises(ValueError, match="channels must be 3"):
        torch_io.check_colour("yuv", "rgb", 1)
    for kw in (dict(channels=1, colour="ycrcb"), dict(channels=3, colour="lab"), dict(channels=3, colour="yuv", order="grb"),
               dict(channels=3, order="grb"), dict(channels=1, colour=2)):
        with pytest.raises(ValueError):
            torch_io.Segmenter(2, 64, 48, **kw)               # refused before any context is created
    doc = torch_io.Segmenter.segment.__doc__
    assert "cvh_convert_colour_batch" in doc and "CONVERTED planes" in doc
    assert "converted planes" in torch_io.Segmenter.images.__doc__


def test_the_proposition_on_the_cpu_oracle():
    """128 x 128, a reddish disk on a greenish ground of the same luma, illumination ramp 0.45 .. 1.45, noise sigma 12.1 from
    synth.splitmix64_stream (colour_util.proposition_image), checkerboard start, default parameters, 600 steps at most.  Measured on
    the oracle (steps, IoU with the disk, better of mask / inverted mask):
        R, G, B     lambda 1, 1, 1     108  0.317   (it segments the ramp)
        Y, Cr, Cb   lambda 1, 1, 1     197  0.212
        Y, Cr, Cb   lambda 0, 1, 1     157  0.989
        Y, Cr, Cb   lambda 0.05, 1, 1  158  0.988
        Y, U, V     lambda 0, 1, 1     181  0.981
    The image is the issue's, re-seeded; nothing about it had to be changed to meet the bars."""
    rows = [U.oracle_proposition(k) for k in range(len(U.PROP_ROWS))]
    for (space, lam), (_, steps, score) in zip(U.PROP_ROWS, rows):
        print(space, lam, steps, round(score, 3))
    assert all(steps < 600 for _, steps, _ in rows)           # every run stopped by its own rule
    assert rows[0][2] <= 0.5
    assert rows[2][2] >= 0.85
