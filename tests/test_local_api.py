"""Local statistics without a GPU: the exported symbols and the header section, the argument errors that need no device, capi's
validation and broadcasting, and the Segmenter's validation.  What needs a device is in test_gpu_local.py."""
import ctypes
import os

import pytest

import local_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvh_local_planes", "cvh_local_planes_batch"]


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    return m


def test_new_symbols_are_exported(capi):
    header = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name) and f"int {name}(" in header
    assert header.index("Colour spaces") < header.index("---- Local statistics") < header.index("---- Energy")
    for text in ("#define CVH_LOCAL_COPY 0", "#define CVH_LOCAL_MEAN 1", "#define CVH_LOCAL_DEV  2", "#define CVH_LOCAL_RADIUS_MAX 127",
                 "(2 S + n) / (2 n)", "isqrt(4 (n Q - S^2) / n^2)"):
        assert text in header
    assert (capi.LOCAL_COPY, capi.LOCAL_MEAN, capi.LOCAL_DEV, capi.LOCAL_RADIUS_MAX) == (U.COPY, U.MEAN, U.DEV, U.RADIUS_MAX) == (0, 1, 2, 127)
    assert callable(capi.local_planes_batch) and callable(capi.Context.local_planes_to)
    L = ctypes.CDLL(capi.LIB_PATH)
    geom = (ctypes.c_int * 3)()
    L.cvh_debug_local_geometry(geom)
    assert list(geom) == [U.BAND, U.STRIP, U.SEGMENT]               # the seam shapes of local_util.CASES are the kernel's
    assert (U.BAND + 1, U.STRIP + 1, 2, "random") in U.CASES and (U.BAND + 1, U.STRIP + 1, U.BAND, "blocky") in U.CASES
    L.cvh_debug_local_launch_sets.restype = ctypes.c_ulong
    assert L.cvh_debug_local_launch_sets() >= 0


def test_argument_errors_without_a_device(capi):
    L = capi.lib()
    err = lambda: L.cvh_last_error(None).decode()
    one, what = (ctypes.c_int * 1)(2), (ctypes.c_int * 3)(0, 1, 2)
    empty = (ctypes.c_void_p * 1)()
    assert L.cvh_local_planes_batch(None, None, 1, one, what) == 1 and "cvh_local_planes_batch" in err()
    assert L.cvh_local_planes_batch(empty, None, 1, one, what) == 1 and "cvh_local_planes_batch" in err()
    assert L.cvh_local_planes_batch(empty, empty, 0, one, what) == 1 and "cvh_local_planes_batch" in err()
    assert L.cvh_local_planes_batch(empty, empty, -3, one, what) == 1 and "cvh_local_planes_batch" in err()
    assert L.cvh_local_planes_batch(empty, empty, 1, one, what) == 1 and "pair 0" in err()
    assert L.cvh_local_planes(None, None, 2, what) == 1 and "cvh_local_planes" in err() and "pair 0" in err()


def test_capi_validates_before_the_library(capi):
    assert capi.local_what_codes("mean") == (1, 1, 1) and capi.local_what_codes("DEV") == (2, 2, 2) and capi.local_what_codes("stack") == (0, 1, 2)
    assert capi.local_what_codes((2,)) == (2, 0, 0) and capi.local_what_codes([1, 0, 2]) == (1, 0, 2)
    for bad in ("var", "", None, 1, (), (0, 1, 2, 0), (3,), (-1, 0, 0), (1.0,), (True,), ("mean",)):
        with pytest.raises(ValueError, match="local statistic"):
            capi.local_what_codes(bad)
    assert capi.local_radius(0) == 0 and capi.local_radius(127) == 127
    for bad in (-1, 128, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="local radius"):
            capi.local_radius(bad)
    ctx = object.__new__(capi.Context)                        # no context is created: the arguments are checked first
    with pytest.raises(ValueError, match="local radius"):
        capi.Context.local_planes_to(ctx, ctx, 128, "dev")
    with pytest.raises(ValueError, match="local statistic"):
        capi.Context.local_planes_to(ctx, ctx, 2, "median")
    with pytest.raises(ValueError, match="pair up"):
        capi.local_planes_batch([], [None], 2, "dev")


def test_batch_broadcasts_a_scalar_radius_and_one_what(capi, monkeypatch):
    """what reaches the library: n radii and 3 n codes, whether given per pair or once"""
    seen = []

    class Lib:
        @staticmethod
        def cvh_local_planes_batch(srcs, dsts, n, radius, what):
            seen.append((n, list(radius)[:n], list(what)[:3 * n]))
            return 0

    class Ctx:
        _h = ctypes.c_void_p(0)

    monkeypatch.setattr(capi, "lib", lambda: Lib)
    a = [Ctx(), Ctx(), Ctx()]
    capi.local_planes_batch(a, a, 4, "stack")
    capi.local_planes_batch(a, a, [1, 2, 3], (2,))
    capi.local_planes_batch(a, a, 0, ["mean", (2, 1, 0), [1]])
    assert seen == [(3, [4, 4, 4], [0, 1, 2] * 3), (3, [1, 2, 3], [2, 0, 0] * 3), (3, [0, 0, 0], [1, 1, 1, 2, 1, 0, 1, 0, 0])]
    for radius, what in (([1, 2], "dev"), (1, ["dev", "mean"]), ([1, 2, 300], "dev"), (1, ["dev", "mean", "max"])):
        with pytest.raises(ValueError):
            capi.local_planes_batch(a, a, radius, what)
    assert len(seen) == 3                                     # refused before the library is reached


def test_segmenter_validates_local_without_a_gpu(capi):
    pytest.importorskip("torch")
    from chan_vese_amd import torch_io
    assert torch_io.check_local(None, 1) is None
    assert torch_io.check_local((2, "dev"), 1) == (2, (2, 2, 2), 1) and torch_io.check_local((3, "mean"), 3) == (3, (1, 1, 1), 3)
    assert torch_io.check_local((2, "stack"), 1) == (2, (0, 1, 2), 3)
    assert torch_io.check_local((0, (2,)), 3) == (0, (2, 0, 0), 1) and torch_io.check_local((127, (2, 2, 1)), 1) == (127, (2, 2, 1), 3)
    with pytest.raises(ValueError, match="channels must be 1"):
        torch_io.check_local((2, "stack"), 3)
    for bad in (2, "dev", (2,), (2, "dev", 1), (128, "dev"), (2, "var"), (2, (1, 2))):
        with pytest.raises(ValueError):
            torch_io.check_local(bad, 1)
    for kw in (dict(channels=3, local=(2, "stack")), dict(channels=1, local=(200, "dev")), dict(channels=1, local="dev")):
        with pytest.raises(ValueError):
            torch_io.Segmenter(2, 64, 48, **kw)               # refused before any context is created
    assert "cvh_local_planes_batch" in torch_io.Segmenter.segment.__doc__ and "LOCAL planes" in torch_io.Segmenter.segment.__doc__
