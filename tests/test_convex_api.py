"""CPU side of the convex-relaxation calls (include/chanvese_hip.h, "Convex relaxation"): the boundary -- header, exports, bindings, the
parameter struct --, what the library refuses before it touches a device, and the partition the sums are taken over."""
import ctypes
import os
import re

import pytest

import multiphase_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cvh_convex_run", "cvh_convex_run_batch", "cvh_get_relaxed", "cvh_get_relaxed_device", "cvh_convex_geometry")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Convex relaxation ----" in hdr
    assert set(re.findall(r"^(?:int|void) (cvh_(?:convex_\w+|get_relaxed\w*))\(", hdr, flags=re.M)) == set(NAMES)
    assert "int cvh_get_relaxed(cvh_context *ctx, double *v, double *qx, double *qy);" in hdr
    assert "int cvh_get_relaxed_device(cvh_context *ctx, double *d_v, void *stream);" in hdr
    section = hdr[hdr.index("---- Convex relaxation"):]
    for said in ("56 bytes per pixel", "8 tau sigma > 1", "vbar' = (v' + v') - v", "u = v - 0.5", "a NaN stays a NaN", "m + n iterations in one call equal m then n"):
        assert said in section, said
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name) and name in capi.EXPORTS
    for name in ("convex_run", "convex_run_batch", "convex_geometry", "make_convex_params"):
        assert callable(getattr(capi, name))
    assert callable(capi.Context.relaxed)


def test_the_struct_is_the_headers(capi, tmp_path):
    """sizeof and the offsets of cvh_convex_params as a C compiler lays them out against the ctypes mirror"""
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "chanvese_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cvh_convex_params), offsetof(cvh_convex_params, tau),\n'
                   "  offsetof(cvh_convex_params, sigma), offsetof(cvh_convex_params, stop_rms), offsetof(cvh_convex_params, means_every),\n"
                   "  offsetof(cvh_convex_params, use_edge), offsetof(cvh_convex_params, resume)); return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()]
    P = capi.ConvexParams
    assert got == [ctypes.sizeof(P)] + [getattr(P, f).offset for f in ("tau", "sigma", "stop_rms", "means_every", "use_edge", "resume")]


def test_ctypes_signatures(capi):
    L = capi.lib()
    vp, ip, dp, ci = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.c_int
    pp = ctypes.POINTER(capi.ConvexParams)
    assert L.cvh_convex_run.argtypes == [vp, ci, pp, ip, dp, dp, ci, ip] and L.cvh_convex_run.restype is ci
    assert L.cvh_convex_run_batch.argtypes == [vp, ci, ci, pp, ip, dp, vp, ci, ip] and L.cvh_convex_run_batch.restype is ci
    assert L.cvh_get_relaxed.argtypes == [vp, dp, dp, dp] and L.cvh_get_relaxed_device.argtypes == [vp, vp, vp]
    assert L.cvh_convex_geometry.argtypes == [ci, ci, ip, ip, ip] and L.cvh_convex_geometry.restype is None


def test_params_marshalling(capi):
    p = capi.make_convex_params(0.25)
    assert (p.tau, p.sigma, p.stop_rms, p.means_every, p.use_edge, p.resume) == (0.25, 0.5, 0.0, 1, 0, 0)   # sigma = 1 / (8 tau)
    p = capi.make_convex_params(tau=0.5, sigma=0.125, stop_rms=-1.0, means_every=0, use_edge=True, resume=True)
    assert (p.tau, p.sigma, p.stop_rms, p.means_every, p.use_edge, p.resume) == (0.5, 0.125, -1.0, 0, 1, 1)
    with pytest.raises(ValueError):
        capi.convex_run_batch([], 1)
    with pytest.raises(TypeError):
        capi.make_convex_params(rho=1.0)


def test_refusals_that_need_no_device(capi):
    L = capi.lib()
    ERR_ARG = 1
    p = capi.make_convex_params(0.25)
    assert L.cvh_convex_run(None, 1, ctypes.byref(p), None, None, None, 0, None) == ERR_ARG
    assert L.cvh_get_relaxed(None, None, None, None) == ERR_ARG and L.cvh_get_relaxed_device(None, None, None) == ERR_ARG
    assert L.cvh_convex_run_batch(None, 1, 1, ctypes.byref(p), None, None, None, 0, None) == ERR_ARG
    assert b"cvh_convex_run_batch: empty member list" in L.cvh_last_error(None)
    one = (ctypes.c_void_p * 1)(None)
    assert L.cvh_convex_run_batch(one, 1, 1, ctypes.byref(p), None, None, None, 0, None) == ERR_ARG
    assert b"member 0 is NULL" in L.cvh_last_error(None)


def test_geometry_is_the_four_phase_partition(capi):
    for h, w, _, _ in M.CASES:
        assert capi.convex_geometry(h, w) == capi.multiphase_geometry(h, w) == (61, M.strip_rows(h, w), -(-h // M.strip_rows(h, w)) * -(-w // 61))
    assert capi.convex_geometry(0, 5)[1:] == (0, 0) and capi.convex_geometry(1 << 14, 1 << 14)[1:] == (0, 0)
