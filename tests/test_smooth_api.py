"""Smoothing without a GPU: the exported symbols and the header section, the constants and the geometry, the argument errors that need
no device, capi's validation and broadcasting, and the Segmenter's validation.  What needs a device is in test_gpu_smooth.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import smooth_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvh_gauss_taps", "cvh_smooth_planes", "cvh_smooth_planes_batch"]


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    return m


def test_new_symbols_are_exported(capi):
    header = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name) and f"int {name}(" in header
    assert "int cvh_smooth_planes(cvh_context *src, cvh_context *dst, int radius, const uint16_t *taps, const int *what);" in header
    assert "int cvh_gauss_taps(double sigma, uint16_t *taps" in header
    assert header.index("---- Local statistics") < header.index("---- Rank planes") < header.index("---- Smoothing") < header.index("---- Energy")
    assert set(capi.EXPORTS) == set(re.findall(r"^[\w \*]+?\b(cvh_\w+)\(", header, flags=re.M))
    section = header[header.index("---- Smoothing"):header.index("---- Energy")]
    for text in ("#define CVH_SMOOTH_COPY   0", "#define CVH_SMOOTH_BLUR   1", "#define CVH_SMOOTH_DETAIL 2", "#define CVH_SMOOTH_RADIUS_MAX 63",
                 "mode='nearest'", "NOT the truncated window", "(a + 64) >> 7", "(b + 2^22) >> 23", "min(255, max(0, 128 + p - BLUR))",
                 "618 below taps[1] = 623", "ceil(3 sigma)"):
        assert text in section, text
    assert '("Smoothing")' in header[header.index("---- Edge-weighted length"):]      # the geodesic section points here
    assert (capi.SMOOTH_COPY, capi.SMOOTH_BLUR, capi.SMOOTH_DETAIL) == (U.COPY, U.BLUR, U.DETAIL) == (0, 1, 2)
    assert capi.SMOOTH_RADIUS_MAX == U.RADIUS_MAX == 63 and capi.SMOOTH_WHATS == U.NAMES
    assert callable(capi.smooth_planes_batch) and callable(capi.Context.smooth_planes_to) and callable(capi.gauss_taps)
    L = ctypes.CDLL(capi.LIB_PATH)
    for R in (0, 1, 30, 63):
        band, strip, segment = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        L.cvh_debug_smooth_geometry(R, ctypes.byref(band), ctypes.byref(strip), ctypes.byref(segment))
        assert (band.value, strip.value, segment.value) == (U.band_rows(R), U.STRIP, U.SEGMENT)      # the seam shapes of smooth_util are the kernels'
    L.cvh_debug_smooth_launch_sets.restype = ctypes.c_ulong
    assert L.cvh_debug_smooth_launch_sets() >= 0


def test_argument_errors_without_a_device(capi):
    L = capi.lib()
    err = lambda: L.cvh_last_error(None).decode()
    one, what = (ctypes.c_int * 1)(1), (ctypes.c_int * 3)(0, 1, 2)
    taps = (ctypes.c_uint16 * 2)(16384, 8192)
    rows = (ctypes.POINTER(ctypes.c_uint16) * 1)(ctypes.cast(taps, ctypes.POINTER(ctypes.c_uint16)))
    empty = (ctypes.c_void_p * 1)()
    assert L.cvh_smooth_planes_batch(None, None, 1, one, rows, what) == 1 and "cvh_smooth_planes_batch" in err()
    assert L.cvh_smooth_planes_batch(empty, None, 1, one, rows, what) == 1 and "cvh_smooth_planes_batch" in err()
    assert L.cvh_smooth_planes_batch(empty, empty, 0, one, rows, what) == 1 and "cvh_smooth_planes_batch" in err()
    assert L.cvh_smooth_planes_batch(empty, empty, -3, one, rows, what) == 1 and "cvh_smooth_planes_batch" in err()
    assert L.cvh_smooth_planes_batch(empty, empty, 1, one, rows, what) == 1 and "pair 0" in err()
    assert L.cvh_smooth_planes(None, None, 1, taps, what) == 1 and "cvh_smooth_planes" in err() and "pair 0" in err()


def test_capi_validates_before_the_library(capi):
    for name, code in U.NAMES.items():
        assert capi.smooth_what_codes(name) == (code,) * 3 == capi.smooth_what_codes(name.upper())
    assert capi.smooth_what_codes((2,)) == (2, 0, 0) and capi.smooth_what_codes([1, 0, 2]) == (1, 0, 2)
    for bad in ("mean", "", None, 1, (), (0, 1, 2, 0), (3,), (-1, 0, 0), (1.0,), (True,), ("blur",)):
        with pytest.raises(ValueError, match="smoothing"):
            capi.smooth_what_codes(bad)
    R, taps = capi.smooth_kernel(1.0)
    assert R == 3 and list(taps) == [13076, 7931, 1770, 145]
    assert capi.smooth_kernel(2)[0] == 6 and list(capi.smooth_kernel(2)[1]) == list(capi.smooth_kernel(2.0)[1])   # a bare integer is a sigma
    R, taps = capi.smooth_kernel([2, 16383])
    assert R == 1 and list(taps) == [2, 16383] and taps.dtype == np.uint16
    assert capi.smooth_kernel(np.array(U.box_taps(63)))[0] == 63 and capi.smooth_kernel((32768,))[0] == 0
    for bad in ((16383, 8192), (), (32768,) + (0,) * 64, (1.5, 2), "blur", None, (True,), (-2, 16385), (32770, -1), 0.0, 22.0, float("nan"), 0, 22, True):
        with pytest.raises(ValueError):
            capi.smooth_kernel(bad)
    ctx = object.__new__(capi.Context)                        # no context is created: the arguments are checked first
    with pytest.raises(ValueError, match="add up"):
        capi.Context.smooth_planes_to(ctx, ctx, [16383, 8192], "blur")
    with pytest.raises(ValueError, match="smoothing"):
        capi.Context.smooth_planes_to(ctx, ctx, 1.0, "dev")
    with pytest.raises(ValueError, match="pair up"):
        capi.smooth_planes_batch([], [None], 1.0, "blur")


def test_batch_broadcasts_one_kernel_and_one_what(capi, monkeypatch):
    """what reaches the library: n radii, n tap lists and 3 n codes, whether given per pair or once"""
    seen = []
    real = capi.lib()

    class Lib:
        cvh_gauss_taps = real.cvh_gauss_taps

        @staticmethod
        def cvh_smooth_planes_batch(srcs, dsts, n, radius, taps, what):
            radii = list(radius)[:n]
            seen.append((n, radii, [[taps[i][j] for j in range(radii[i] + 1)] for i in range(n)], list(what)[:3 * n]))
            return 0

    class Ctx:
        _h = ctypes.c_void_p(0)
        channels = 3

    monkeypatch.setattr(capi, "lib", lambda: Lib)
    a = [Ctx(), Ctx(), Ctx()]
    g1, g2 = list(U.gauss_taps(1.0)[1]), list(U.gauss_taps(0.5)[1])
    capi.smooth_planes_batch(a, a, 1.0, "detail")
    capi.smooth_planes_batch(a, a, [2, 16383], (1,))
    capi.smooth_planes_batch(a, a, [1.0, [32768], 0.5], ["blur", (2, 1, 0), [1]])
    assert seen == [(3, [3, 3, 3], [g1] * 3, [2, 2, 2] * 3), (3, [1, 1, 1], [[2, 16383]] * 3, [1, 0, 0] * 3),
                    (3, [3, 0, 2], [g1, [32768], g2], [1, 1, 1, 2, 1, 0, 1, 0, 0])]
    for kernel, what in (([1.0, 2.0], "blur"), (1.0, ["blur", "detail"]), ([1.0, 2.0, 30.0], "blur"), (1.0, ["blur", "detail", "dev"]),
                         ([[2, 16383], [2, 16384], [32768]], "blur")):
        with pytest.raises(ValueError):
            capi.smooth_planes_batch(a, a, kernel, what)
    assert len(seen) == 3                                     # refused before the library is reached


def test_segmenter_validates_smooth_and_edge_sigma_without_a_gpu(capi):
    pytest.importorskip("torch")
    from chan_vese_amd import torch_io
    assert torch_io.check_smooth(None, 1) is None
    (R, taps), codes, made = torch_io.check_smooth((1.5, "blur"), 1)
    assert (R, tuple(int(t) for t in taps), codes, made) == (5, U.gauss_taps(1.5)[1], (1, 1, 1), 1)
    assert torch_io.check_smooth((2, "blur"), 1)[0][0] == 6                            # an int sigma, as edge_sigma=2
    assert torch_io.check_smooth(([2, 16383], (0, 1, 2)), 1)[1:] == ((0, 1, 2), 3) and torch_io.check_smooth((2.0, "detail"), 3)[1:] == ((2, 2, 2), 3)
    for bad in (1.5, "blur", (1.5,), (1.5, "blur", 1), (0.0, "blur"), (30.0, "blur"), (1.5, "dev"), (1.5, (1, 2)), ([1, 2], "blur")):
        with pytest.raises(ValueError):
            torch_io.check_smooth(bad, 1)
    assert torch_io.check_edge_sigma(None, None) is None and torch_io.check_edge_sigma(None, 5.0) is None
    assert torch_io.check_edge_sigma(2, 5.0)[0] == 6
    for sigma, edge in ((2.0, None), (0.0, 5.0), (-1.0, 5.0), (22.0, 5.0), (float("nan"), 5.0), ("2", 5.0), (True, 5.0)):
        with pytest.raises(ValueError, match="edge_sigma"):
            torch_io.check_edge_sigma(sigma, edge)
    for kw in (dict(channels=1, smooth=(30.0, "blur")), dict(channels=1, smooth="blur"), dict(channels=1, smooth=(1.0, "blur"), phases=4),
               dict(channels=3, smooth=(1.0, "blur"), local=(2, "stack")),           # the stack needs ONE plane behind the blur
               dict(channels=1, edge_sigma=2.0), dict(channels=1, edge=5.0, edge_sigma=0.0)):
        with pytest.raises(ValueError):
            torch_io.Segmenter(2, 64, 48, **kw)               # refused before any context is created
    assert "cvh_smooth_planes_batch" in torch_io.Segmenter.segment.__doc__ and "SMOOTHED planes" in torch_io.Segmenter.segment.__doc__
