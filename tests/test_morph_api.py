"""CPU side of the mask morphology (include/chanvese_hip.h, "Mask morphology"): the boundary -- header, exports, constants, what is
refused before a device is touched, the squared radius of the Python drivers -- and the trips of the one new kernel whose grid is capped,
read from the library."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import morph_util as M
import trips_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cvh_get_mask_morph", "cvh_get_mask_morph_device", "cvh_get_mask_morph_device_batch", "cvh_morph_levelset", "cvh_morph_levelset_batch",
       "cvh_init_mask", "cvh_init_mask_device", "cvh_init_mask_device_batch")
TRIPS_MORPH_EMIT = 16


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Mask morphology ----" in hdr
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", hdr), name
    assert re.search(r"int cvh_get_mask_morph_device_batch\(cvh_context \*const \*ctxs, int n, uint8_t \*const \*d_masks, int conn, int invert, "
                     r"long min_area,\s+long fill_holes, int keep_largest, int op, const uint32_t \*r2, void \*stream\);", hdr)
    assert re.search(r"int cvh_init_mask_device\(cvh_context \*ctx, const uint8_t \*d_mask, double inside, double outside, void \*stream\);", hdr)
    for k, name in enumerate(("NONE", "DILATE", "ERODE", "OPEN", "CLOSE")):
        assert re.search(r"#define CVH_MORPH_%s\s+%d\b" % (name, k), hdr), name
        assert getattr(capi, "MORPH_" + name) == k == getattr(M, name) and capi.MORPH_OPS[name.lower()] == k
    for text in ("dx^2 + dy^2 <= r2", "P \\ dilate(P \\ F)", "binary_dilation(F, disk, border_value=0)", "binary_erosion(F, disk, border_value=1)",
                 "3.25 bytes per pixel", "h^2 + w^2 >= 2^32"):
        assert text in hdr, text
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name) and name in capi.EXPORTS, name
    raw.cvh_debug_morph_launch_sets.restype = ctypes.c_ulong
    assert raw.cvh_debug_morph_launch_sets() >= 0


def test_r2_of_is_the_floor_of_the_square(capi):
    assert [capi.r2_of(r) for r in (0, 0.99, 1, 1.5, 2.0, 2.5, math.sqrt(2), 3, 20)] == [0, 0, 1, 2, 4, 6, 2, 9, 400]
    assert capi.r2_of(1e9) == 0xFFFFFFFF and capi.r2_of(65535) == 65535 ** 2 and capi.r2_of(65536) == 0xFFFFFFFF
    for bad in (-1, -1e-9, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError):
            capi.r2_of(bad)
    assert [capi.morph_code(v) for v in (None, "none", "Dilate", "erode", "open", "CLOSE", 3)] == [0, 0, 1, 2, 3, 4, 3]
    with pytest.raises(ValueError):
        capi.morph_code("thin")


def test_null_arguments_are_refused_without_a_device(capi):
    """what the library refuses before it touches a device: a NULL context, a NULL or empty list"""
    L = capi.lib()
    ptrs = (ctypes.c_void_p * 1)(None)
    r2 = (ctypes.c_uint32 * 1)(1)
    assert L.cvh_get_mask_morph(None, None, 4, 0, 0, 0, 0, 1, 1) != capi.CVH_OK
    assert L.cvh_get_mask_morph_device(None, None, 4, 0, 0, 0, 0, 1, 1, None) != capi.CVH_OK
    assert L.cvh_morph_levelset(None, 4, 0, 0, 0, 0, 1, 1, 1.0, -1.0) != capi.CVH_OK
    assert L.cvh_init_mask(None, None, 1.0, -1.0) != capi.CVH_OK and L.cvh_init_mask_device(None, None, 1.0, -1.0, None) != capi.CVH_OK
    for ctxs, n in ((None, 1), ((ctypes.c_void_p * 1)(None), 1), ((ctypes.c_void_p * 1)(None), 0)):
        assert L.cvh_get_mask_morph_device_batch(ctxs, n, ptrs, 4, 0, 0, 0, 0, 1, r2, None) != capi.CVH_OK
        assert b"cvh_get_mask_morph_device_batch" in L.cvh_last_error(None)
        assert L.cvh_morph_levelset_batch(ctxs, n, 4, 0, 0, 0, 0, 1, r2, 1.0, -1.0) != capi.CVH_OK
        assert b"cvh_morph_levelset_batch" in L.cvh_last_error(None)
        assert L.cvh_init_mask_device_batch(ctxs, n, ptrs, 1.0, -1.0, None) != capi.CVH_OK
        assert b"cvh_init_mask_device_batch" in L.cvh_last_error(None)
    for call in (lambda: capi.mask_morph_batch([], [], M.OPEN, r2=1), lambda: capi.morph_levelset_batch([], M.OPEN, r2=1), lambda: capi.init_mask_batch([], [])):
        with pytest.raises(capi.CvhError):
            call()


def test_morph_without_gpu_fails_as_other_calls_do(capi):
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CvhError) as e:
        capi.Context(16, 16).init_mask(np.zeros((16, 16), np.uint8))
    assert "no HIP device" in str(e.value)


def test_the_emit_launch_makes_a_second_trip_where_the_gpu_test_runs_it(capi):
    """the one new kernel with a capped grid, at the shape test_gpu_morph.py uses: two trips, the seam inside the plane, a ragged tail;
    the column and row launches of a pass take one band x chunk slot per workgroup (uncapped: the reinitialisation's column grid)"""
    h, w = T.IO_SHAPE
    items, nblk, takers = T.counts(TRIPS_MORPH_EMIT, h, w)
    assert T.trips(TRIPS_MORPH_EMIT, h, w) >= 2 and items > nblk * takers and (h * w) % 16 == 1
    assert T.first_trip(TRIPS_MORPH_EMIT, h, w) * 16 < h * w
    assert T.trips(TRIPS_MORPH_EMIT, 96, 300) == 1                      # the everyday shapes stay below the cap
    for hh, ww in M.SHAPES + [(300, 40), (3, 8200), T.IO_SHAPE]:
        assert T.trips(T.COLUMNS, hh, ww) == 1
    fn = ctypes.CDLL(capi.LIB_PATH).cvh_debug_trip_counts
    out = (ctypes.byref(ctypes.c_ulonglong()), ctypes.byref(ctypes.c_uint()), ctypes.byref(ctypes.c_uint()))
    assert all(fn(op, 4, 4, *out) == 1 for op in (8, 15, 17)) and fn(16, 4, 4, *out) == 0   # the old codes keep their numbers, 8 stays refused
