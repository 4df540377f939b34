"""CPU side of the edge-weighted calls (include/chanvese_hip.h, "Edge-weighted length"): the boundary -- header, exports, bindings --,
what the library refuses before it touches a device, and the partition the sums are taken over (pure host arithmetic)."""
import ctypes
import os
import re

import pytest

import geodesic_util as G
import multiphase_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cvh_set_edge_map", "cvh_get_edge_map", "cvh_set_edge_map_device", "cvh_get_edge_map_device", "cvh_edge_map", "cvh_edge_map_batch",
         "cvh_geodesic_run", "cvh_geodesic_run_batch", "cvh_geodesic_geometry")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Edge-weighted length ----" in hdr
    assert set(re.findall(r"^(?:int|void) (cvh_(?:\w*edge_map\w*|geodesic_\w+))\(", hdr, flags=re.M)) == set(NAMES)
    assert "int cvh_set_edge_map(cvh_context *ctx, const uint16_t *gq);" in hdr
    assert "int cvh_set_edge_map_device(cvh_context *ctx, const uint16_t *d_gq, void *stream);" in hdr
    assert "int cvh_edge_map(cvh_context *dst, cvh_context *src, double K);" in hdr
    assert "int cvh_geodesic_run(cvh_context *ctx, int max_steps, int *steps_done, double *norm, double *trace, int trace_rows, int *rows);" in hdr
    section = hdr[hdr.index("---- Edge-weighted length"):]
    for said in ("do NOT touch it", "CLAMP", "There is no Gaussian", "cvh_energy does not know g", "rint(32768.0 / (1.0 + (double)m2 / den))"):
        assert said in section, said
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in capi.EXPORTS
    for name in ("geodesic_run", "geodesic_run_batch", "geodesic_geometry", "edge_map_batch"):
        assert callable(getattr(capi, name))
    for name in ("set_edge_map", "get_edge_map", "edge_map_from"):
        assert callable(getattr(capi.Context, name))


def test_ctypes_signatures(capi):
    L = capi.lib()
    vp, ip, dp, ci, cd = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_double
    assert L.cvh_set_edge_map.argtypes == [vp, vp] and L.cvh_get_edge_map.argtypes == [vp, vp]
    assert L.cvh_set_edge_map_device.argtypes == [vp, vp, vp] and L.cvh_get_edge_map_device.argtypes == [vp, vp, vp]
    assert L.cvh_edge_map.argtypes == [vp, vp, cd] and L.cvh_edge_map.restype is ci
    assert L.cvh_edge_map_batch.argtypes == [vp, vp, ci, dp] and L.cvh_edge_map_batch.restype is ci
    assert L.cvh_geodesic_run.argtypes == [vp, ci, ip, dp, dp, ci, ip] and L.cvh_geodesic_run.restype is ci
    assert L.cvh_geodesic_run_batch.argtypes == [vp, ci, ci, ip, dp, vp, ci, ip] and L.cvh_geodesic_run_batch.restype is ci
    assert L.cvh_geodesic_geometry.argtypes == [ci, ci, ip, ip, ip] and L.cvh_geodesic_geometry.restype is None


def test_refusals_that_need_no_device(capi):
    L = capi.lib()
    ERR_ARG = 1
    buf = (ctypes.c_uint16 * 4)()
    assert L.cvh_geodesic_run(None, 1, None, None, None, 0, None) == ERR_ARG
    assert L.cvh_geodesic_run_batch(None, 0, 1, None, None, None, 0, None) == ERR_ARG
    assert L.cvh_set_edge_map(None, buf) == ERR_ARG and L.cvh_get_edge_map(None, buf) == ERR_ARG
    assert L.cvh_set_edge_map_device(None, buf, None) == ERR_ARG and L.cvh_get_edge_map_device(None, buf, None) == ERR_ARG
    for K in (30.0, 0.0, -1.0):
        assert L.cvh_edge_map(None, None, K) == ERR_ARG
    assert "is NULL" in L.cvh_last_error(None).decode()
    assert L.cvh_edge_map_batch(None, None, 0, None) == ERR_ARG and "empty pair list" in L.cvh_last_error(None).decode()
    with pytest.raises(ValueError):
        capi.geodesic_run(None, max_steps=-1, trace=True)   # all rows of an unbounded run: refused before the library is reached


def test_partition(capi):
    """the four-phase partition: 61 output columns per wave, strips of a multiple of four rows, at least 8, for about 4096 waves"""
    g = capi.geodesic_geometry
    assert g(9, 130) == (61, 8, 6) and g(24, 64) == (61, 8, 6) and g(4096, 4096) == (61, 72, 57 * 68)
    for bad in ((1 << 14, 1 << 14), (0, 5), (5, 0)):
        assert g(*bad)[1:] == (0, 0)
    for h, w, _, _ in M.CASES:
        cols, rows, items = g(h, w)
        assert (cols, rows) == (61, M.strip_rows(h, w)) and items == -(-h // rows) * -(-w // 61)
        assert g(h, w) == capi.multiphase_geometry(h, w)
    assert len(G.CASES) == 2 * len(M.CASES)
