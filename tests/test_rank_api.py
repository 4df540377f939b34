"""Rank planes without a GPU: the exported symbols and the header section, the constants and the geometry in the header, the library
and rank_util, the argument errors that need no device, capi's validation and broadcasting, and the Segmenter's validation.  What needs
a device is in test_gpu_rank.py."""
import ctypes
import os

import pytest

import rank_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvh_rank_planes", "cvh_rank_planes_batch"]


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    return m


def test_new_symbols_are_exported(capi):
    header = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    internal = open(os.path.join(ROOT, "chan_vese_amd", "csrc", "cvh_internal.h")).read()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name) and f"int {name}(" in header
    assert "int cvh_rank_planes(cvh_context *src, cvh_context *dst, int radius, const int *what);" in header
    assert header.index("---- Local statistics") < header.index("---- Rank planes") < header.index("---- Energy")
    for text in ("#define CVH_RANK_COPY   0", "#define CVH_RANK_MIN    1", "#define CVH_RANK_MAX    2", "#define CVH_RANK_MEDIAN 3",
                 "#define CVH_RANK_OPEN   4", "#define CVH_RANK_CLOSE  5", "#define CVH_RANK_TOPHAT 6", "#define CVH_RANK_BOTHAT 7",
                 "#define CVH_RANK_RADIUS_MAX        127", "#define CVH_RANK_MEDIAN_RADIUS_MAX 7", "s[(n-1)/2]", "OPEN <= p <= CLOSE",
                 "need no clamp"):
        assert text in header, text
    assert (capi.RANK_COPY, capi.RANK_MIN, capi.RANK_MAX, capi.RANK_MEDIAN, capi.RANK_OPEN, capi.RANK_CLOSE, capi.RANK_TOPHAT,
            capi.RANK_BOTHAT) == U.CODES == tuple(range(8))
    assert (capi.RANK_RADIUS_MAX, capi.RANK_MEDIAN_RADIUS_MAX) == (U.RADIUS_MAX, U.MEDIAN_RADIUS_MAX) == (127, 7)
    assert capi.RANK_WHATS == U.NAMES
    assert callable(capi.rank_planes_batch) and callable(capi.Context.rank_planes_to)
    L = ctypes.CDLL(capi.LIB_PATH)
    geom = (ctypes.c_int * 5)()
    L.cvh_debug_rank_geometry(geom)
    assert list(geom) == [U.BAND, U.STRIP, U.SEGMENT, U.MEDIAN_BAND, U.MEDIAN_STRIP]      # the seam shapes of rank_util are the kernels'
    assert "#define CVH_RANK_SEGMENT CVH_LOCAL_SEGMENT" in internal and "#define CVH_RANK_BAND CVH_LOCAL_BAND" in internal
    assert (U.BAND + 1, U.STRIP + 1, 2, "random") in U.CASES and (U.BAND + 1, U.STRIP + 1, U.BAND, "blocky") in U.CASES
    assert (3, U.SEGMENT + 1, 5, "random") in U.CASES and (2, U.SEGMENT + 7, 127, "blocky") in U.CASES
    assert (U.MEDIAN_BAND + 1, U.STRIP + 1, 7, "blocky") in U.MEDIAN_CASES
    assert [L.cvh_debug_rank_band_rows(R) for R in (0, 2, 32, 127)] == [U.band_rows(R) for R in (0, 2, 32, 127)] == [32, 35, 65, 255]
    L.cvh_debug_rank_launch_sets.restype = ctypes.c_ulong
    assert L.cvh_debug_rank_launch_sets() >= 0


def test_argument_errors_without_a_device(capi):
    L = capi.lib()
    err = lambda: L.cvh_last_error(None).decode()
    one, what = (ctypes.c_int * 1)(2), (ctypes.c_int * 3)(0, 1, 2)
    empty = (ctypes.c_void_p * 1)()
    assert L.cvh_rank_planes_batch(None, None, 1, one, what) == 1 and "cvh_rank_planes_batch" in err()
    assert L.cvh_rank_planes_batch(empty, None, 1, one, what) == 1 and "cvh_rank_planes_batch" in err()
    assert L.cvh_rank_planes_batch(empty, empty, 0, one, what) == 1 and "cvh_rank_planes_batch" in err()
    assert L.cvh_rank_planes_batch(empty, empty, -3, one, what) == 1 and "cvh_rank_planes_batch" in err()
    assert L.cvh_rank_planes_batch(empty, empty, 1, one, what) == 1 and "pair 0" in err()
    assert L.cvh_rank_planes(None, None, 2, what) == 1 and "cvh_rank_planes" in err() and "pair 0" in err()


def test_capi_validates_before_the_library(capi):
    for name, code in U.NAMES.items():
        assert capi.rank_what_codes(name) == (code,) * 3 == capi.rank_what_codes(name.upper())
    assert capi.rank_what_codes((6,)) == (6, 0, 0) and capi.rank_what_codes([3, 0, 7]) == (3, 0, 7)
    for bad in ("mean", "", None, 1, (), (0, 1, 2, 0), (8,), (-1, 0, 0), (1.0,), (True,), ("median",)):
        with pytest.raises(ValueError, match="rank filter"):
            capi.rank_what_codes(bad)
    assert capi.rank_radius(0) == 0 and capi.rank_radius(127) == 127 and capi.rank_radius(7, (3, 0, 0)) == 7
    assert capi.rank_radius(127, (1, 2, 4)) == 127
    for bad in (-1, 128, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="rank radius"):
            capi.rank_radius(bad)
    with pytest.raises(ValueError, match="for a median"):
        capi.rank_radius(8, (0, 3, 0))
    ctx = object.__new__(capi.Context)                        # no context is created: the arguments are checked first
    with pytest.raises(ValueError, match="rank radius"):
        capi.Context.rank_planes_to(ctx, ctx, 128, "open")
    with pytest.raises(ValueError, match="for a median"):
        capi.Context.rank_planes_to(ctx, ctx, 8, "median")
    with pytest.raises(ValueError, match="rank filter"):
        capi.Context.rank_planes_to(ctx, ctx, 2, "dev")
    with pytest.raises(ValueError, match="pair up"):
        capi.rank_planes_batch([], [None], 2, "open")


def test_batch_broadcasts_a_scalar_radius_and_one_what(capi, monkeypatch):
    """what reaches the library: n radii and 3 n codes, whether given per pair or once"""
    seen = []

    class Lib:
        @staticmethod
        def cvh_rank_planes_batch(srcs, dsts, n, radius, what):
            seen.append((n, list(radius)[:n], list(what)[:3 * n]))
            return 0

    class Ctx:
        _h = ctypes.c_void_p(0)
        channels = 3

    class Grey(Ctx):
        channels = 1

    monkeypatch.setattr(capi, "lib", lambda: Lib)
    a = [Ctx(), Ctx(), Ctx()]
    capi.rank_planes_batch(a, a, 4, "tophat")
    capi.rank_planes_batch(a, a, [1, 2, 3], (3,))
    capi.rank_planes_batch(a, a, 0, ["median", (2, 1, 0), [5]])
    capi.rank_planes_batch(a, [Grey(), Grey(), Grey()], 100, (1, 3, 3))          # a median behind the destination's planes binds nothing
    assert seen == [(3, [4, 4, 4], [6, 6, 6] * 3), (3, [1, 2, 3], [3, 0, 0] * 3), (3, [0, 0, 0], [3, 3, 3, 2, 1, 0, 5, 0, 0]),
                    (3, [100] * 3, [1, 3, 3] * 3)]
    for radius, what in (([1, 2], "open"), (1, ["open", "min"]), ([1, 2, 300], "open"), (1, ["open", "min", "dev"]), ([1, 2, 8], "median"),
                         (8, (1, 3, 3))):
        with pytest.raises(ValueError):
            capi.rank_planes_batch(a, a, radius, what)
    assert len(seen) == 4                                     # refused before the library is reached


def test_segmenter_validates_rank_without_a_gpu(capi):
    pytest.importorskip("torch")
    from chan_vese_amd import torch_io
    assert torch_io.check_rank(None, 1) is None
    assert torch_io.check_rank((2, "median"), 1) == (2, (3, 3, 3), 1) and torch_io.check_rank((30, "tophat"), 3) == (30, (6, 6, 6), 3)
    assert torch_io.check_rank((0, (2,)), 3) == (0, (2, 0, 0), 1) and torch_io.check_rank((127, (0, 4, 6)), 1) == (127, (0, 4, 6), 3)
    assert torch_io.check_rank((20, (1, 3, 3)[:1]), 1) == (20, (1, 0, 0), 1)
    for bad in (2, "open", (2,), (2, "open", 1), (128, "open"), (8, "median"), (2, "dev"), (2, (1, 2)), (9, (0, 3, 0))):
        with pytest.raises(ValueError):
            torch_io.check_rank(bad, 1)
    for kw in (dict(channels=1, rank=(200, "open")), dict(channels=1, rank="open"), dict(channels=3, rank=(8, "median")),
               dict(channels=3, rank=(1, "median"), local=(2, "stack"))):          # the stack needs ONE plane behind the rank filter
        with pytest.raises(ValueError):
            torch_io.Segmenter(2, 64, 48, **kw)               # refused before any context is created
    assert "cvh_rank_planes_batch" in torch_io.Segmenter.segment.__doc__ and "RANK planes" in torch_io.Segmenter.segment.__doc__
