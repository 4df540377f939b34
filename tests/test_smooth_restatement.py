"""The smoothing definition without a GPU (include/chanvese_hip.h, "Smoothing"): the two restatements of smooth_util against each other,
the properties that follow from the arithmetic, the widths of the intermediates, the roundings of smooth_math.h compiled for the host,
cvh_gauss_taps against the header's formula in numpy, and a sanity check against scipy's own Gaussian.  What needs a device is in
test_gpu_smooth.py."""
import ctypes
import math

import numpy as np
import pytest

import smooth_util as U


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    return m


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (5, 7), (40, 50), (70, 130)])
def test_the_two_restatements_agree(shape):
    for seed, (name, R) in enumerate((("gauss", 0), ("gauss", 1), ("gauss", 5), ("box", 3), ("rim", 1), ("rim", 63), ("gauss", 63), ("box", 63))):
        taps = U.kernel_of(name, R)
        for kind in ("random", "blocky"):
            p = U.planes_of(kind, *shape, 1, seed)[0]
            assert np.array_equal(U.blur(p, taps), U.blur_scipy(p, taps)), (name, R, kind)


def test_properties_that_follow_from_the_arithmetic():
    p = U.planes_of("random", 23, 31, 1, 5)[0]
    assert np.array_equal(U.blur(p, (U.TAP_SUM,)), p)                                # R = 0 is the identity
    for name, R in (("gauss", 4), ("box", 7), ("rim", 63), ("gauss", 63)):
        taps = U.kernel_of(name, R)
        for c in (0, 1, 77, 128, 254, 255):
            flat = np.full((9, 11), c, np.uint8)
            assert (U.blur(flat, taps) == c).all() and (U.detail(flat, U.blur(flat, taps)) == 128).all()
    assert U.box_taps(3) == (4682,) + (4681,) * 3 and U.kernel_of("rim", 1) == (2, 16383)
    want = U.expected([p], 3, U.kernel_of("box", 2), (U.COPY, U.BLUR, U.DETAIL))
    assert np.array_equal(want[0], p) and np.array_equal(want[2], np.clip(128 + p.astype(int) - want[1].astype(int), 0, 255))


def test_no_intermediate_leaves_its_width():
    white = np.full((130, 140), 255, np.uint8)
    for name in ("gauss", "box", "rim"):
        taps = U.kernel_of(name, 63)
        a = U.row_sums(white, taps)
        assert a.max() == 255 * 32768 < 1 << 23
        v = (a + 64) >> 7
        assert v.max() == 65280 <= 0xffff
        b = U.column_sums(v, taps)
        assert b.max() == 65280 * 32768 < 1 << 31
        assert ((b + (1 << 22)) >> 23).max() == 255


def test_the_roundings_compiled_for_the_host(capi):
    L = ctypes.CDLL(capi.LIB_PATH)
    for f in (L.cvh_debug_smooth_row, L.cvh_debug_smooth_blur, L.cvh_debug_smooth_detail):
        f.restype = ctypes.c_uint
    for a in (0, 63, 64, 191, 192, 255 * 32768, 12345678 % (1 << 23)):
        assert L.cvh_debug_smooth_row(a) == (a + 64) >> 7
    for b in (0, (1 << 22) - 1, 1 << 22, 3 << 22, 65280 * 32768, 77 * 256 * 32768):
        assert L.cvh_debug_smooth_blur(b) == (b + (1 << 22)) >> 23
    for p in (0, 1, 127, 128, 200, 255):
        for q in (0, 1, 127, 128, 200, 255):
            assert L.cvh_debug_smooth_detail(p, q) == min(255, max(0, 128 + p - q))


SIGMAS = (0.3, 0.5, 1, 1.5, 2, 3.7, 10, 21)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_gauss_taps_are_the_formula(capi, sigma):
    """The library's taps EQUAL numpy's at every sigma of the list (measured, and asserted with ==): both evaluate the same doubles"""
    R, taps = capi.gauss_taps(sigma)
    want_R, want = U.gauss_taps(float(sigma))
    assert R == want_R == math.ceil(3 * sigma) and len(taps) == R + 1 and taps.dtype == np.uint16
    assert int(taps[0]) + 2 * int(taps[1:].astype(np.int64).sum()) == U.TAP_SUM
    print(sigma, "largest difference of a tap from numpy's:", int(np.abs(taps.astype(np.int64) - np.array(want)).max()))
    assert tuple(int(t) for t in taps) == want


def test_gauss_taps_centre_absorbs_the_residue_and_refusals(capi):
    R, taps = capi.gauss_taps(21)
    assert R == 63 and (int(taps[0]), int(taps[1])) == (618, 623)                    # the header says so: expected, and legal
    L = capi.lib()
    buf, r = (ctypes.c_uint16 * 64)(), ctypes.c_int(-7)
    for bad in (0.0, -1.0, 21.0000001, 1e9, float("nan"), float("inf"), -float("inf")):
        assert L.cvh_gauss_taps(bad, buf, ctypes.byref(r)) == 1 and "cvh_gauss_taps" in L.cvh_last_error(None).decode()
        assert r.value == -7
        with pytest.raises(ValueError, match="sigma"):
            capi.gauss_taps(bad)
    assert L.cvh_gauss_taps(1.0, None, ctypes.byref(r)) == 1 and "NULL" in L.cvh_last_error(None).decode()
    assert L.cvh_gauss_taps(1.0, buf, None) == 1 and "NULL" in L.cvh_last_error(None).decode()
    assert L.cvh_gauss_taps(1.0, buf, ctypes.byref(r)) == 0 and r.value == 3 and list(buf[:6]) == [13076, 7931, 1770, 145, 0, 0]
    for bad in ("1", None, True, [1.0]):
        with pytest.raises(ValueError):
            capi.gauss_taps(bad)


@pytest.mark.parametrize("sigma", [0.5, 1, 1.5, 2, 3.7, 10])
def test_blur_is_within_a_grey_level_of_scipys_gaussian(capi, sigma):
    """A check, not the contract.  Budget: 0.5 for the last rounding, 1/512 for the row rounding, at most (2 R + 1) 0.5 / 32768 * 255 =
    0.24 for the tap rounding at R = 30"""
    from scipy import ndimage
    p = U.planes_of("random", 40, 50, 1, 9)[0]
    ref = ndimage.gaussian_filter(p.astype(np.float64), sigma, mode="nearest", truncate=3.0)
    got = U.blur(p, capi.gauss_taps(sigma)[1])
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("sigma", sigma, "largest distance from scipy's gaussian_filter:", err)
    assert err <= 1.0
