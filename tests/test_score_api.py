"""CPU side of the mask scores (include/chanvese_hip.h, "Mask scores"): the boundary -- header, exports, the ctypes struct against the C
struct, what is refused before a device is touched, the derived figures and the tolerance of the Python drivers -- and the restatement
(score_util.py) against facts that do not depend on it."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import score_util as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Mask scores ----" in hdr
    assert re.search(r"int cvh_score_mask\(cvh_context \*ctx, const uint8_t \*truth, int invert, uint32_t tol2, cvh_mask_score \*out\);", hdr)
    assert re.search(r"int cvh_score_mask_device\(cvh_context \*ctx, const uint8_t \*d_truth, int invert, uint32_t tol2, cvh_mask_score \*out, "
                     r"void \*stream\);", hdr)
    assert re.search(r"int cvh_score_mask_device_batch\(cvh_context \*const \*ctxs, int n, const uint8_t \*const \*d_truths, int invert, "
                     r"uint32_t tol2,\s+cvh_mask_score \*out, void \*stream\);", hdr)
    for text in ("llrint(sqrt((double)d2) * 65536)", "iou = tp / (tp + fp + fn)", "dice = 2 tp / (2 tp + fp + fn)",
                 "hausdorff = sqrt(max(hd2_m, hd2_t))", "assd = (dist_m_q16 + dist_t_q16) / 65536 / (surf_m + surf_t)",
                 "surface_dice = (within_m + within_t) / (surf_m + surf_t)", "h^2 + w^2 < 2^32 and h w < 2^31"):
        assert text in hdr, text
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in ("cvh_score_mask", "cvh_score_mask_device", "cvh_score_mask_device_batch"):
        assert hasattr(raw, name) and name in capi.EXPORTS
    raw.cvh_debug_score_launch_sets.restype = ctypes.c_ulong
    assert raw.cvh_debug_score_launch_sets() >= 0


def test_struct_layout_matches_the_header(capi, tmp_path):
    """the ctypes struct and the C struct agree on size and on every offset"""
    fields = [f for f, _ in capi.MaskScore._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include "chanvese_hip.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                   'int main(void) { printf("%zu", sizeof(cvh_mask_score));\n'
                   + "".join(f'  printf(" %zu", offsetof(cvh_mask_score, {f}));\n' for f in fields) + '  printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()]
    T = capi.MaskScore
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields] and got[0] == 96
    assert fields == ["tp", "fp", "fn", "tn", "surf_m", "surf_t", "within_m", "within_t", "dist_m_q16", "dist_t_q16", "hd2_m", "hd2_t", "defined", "pad"]


def test_null_arguments_are_refused_without_a_device(capi):
    """what the library refuses before it touches a device: a NULL context, a NULL or empty list"""
    L = capi.lib()
    out = (capi.MaskScore * 1)()
    ptrs = (ctypes.c_void_p * 1)(None)
    assert L.cvh_score_mask(None, None, 0, 4, out) != capi.CVH_OK
    assert L.cvh_score_mask_device(None, None, 0, 4, out, None) != capi.CVH_OK
    for ctxs, n in ((None, 1), ((ctypes.c_void_p * 1)(None), 1), ((ctypes.c_void_p * 1)(None), 0)):
        assert L.cvh_score_mask_device_batch(ctxs, n, ptrs, 0, 4, out, None) != capi.CVH_OK
        assert b"cvh_score_mask_device_batch" in L.cvh_last_error(None)
    with pytest.raises(capi.CvhError):
        capi.score_batch([], [])


def test_score_without_gpu_fails_as_other_calls_do(capi):
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CvhError) as e:
        capi.Context(16, 16).score(np.zeros((16, 16), np.uint8))
    assert "no HIP device" in str(e.value)


# ---- the Python drivers' own arithmetic ----
def test_tol2_is_the_floor_of_the_square(capi):
    assert [capi.score_tol2(t) for t in (0, 0.99, 1, 1.5, 2.0, 2.5, math.sqrt(2), 3)] == [0, 0, 1, 2, 4, 6, 2, 9]
    assert capi.score_tol2(1e9) == 0xFFFFFFFF
    for bad in (-1, float("nan"), float("inf"), "2", None, True):
        with pytest.raises(ValueError):
            capi.score_tol2(bad)


def test_derived_properties(capi):
    s = capi.Score(tp=30, fp=10, fn=20, tn=40, surf_m=8, surf_t=12, within_m=6, within_t=9, dist_m_q16=3 * 65536, dist_t_q16=7 * 65536 + 32768,
                   hd2_m=25, hd2_t=9, defined=1)
    assert s.iou == 30 / 60 and s.dice == 60 / 90 and s.hausdorff == 5.0 and s.assd == 10.5 / 20 and s.surface_dice == 15 / 20
    # a surface is empty: the boundary figures are NaN, the overlap figures are not
    e = capi.Score(tp=0, fp=10, fn=0, tn=90, surf_m=9, surf_t=0, within_m=0, within_t=0, dist_m_q16=0, dist_t_q16=0, hd2_m=0, hd2_t=0, defined=0)
    assert e.iou == 0.0 and e.dice == 0.0 and all(math.isnan(v) for v in (e.hausdorff, e.assd, e.surface_dice))
    # nothing anywhere: every denominator is 0
    z = capi.Score(*([0] * 3), 100, *([0] * 9))
    assert all(math.isnan(v) for v in (z.iou, z.dice, z.hausdorff, z.assd, z.surface_dice))
    assert tuple(f.name for f in __import__("dataclasses").fields(capi.Score)) == S.FIELDS == capi.SCORE_FIELDS


def test_score_of_a_struct(capi):
    m = capi.MaskScore()
    for k, f in enumerate(S.FIELDS):
        setattr(m, f, k + 1)
    m.dist_t_q16 = 2 ** 63 + 5                                       # the sums are unsigned 64-bit
    assert S.as_dict(capi._score_of(m)) == {**{f: k + 1 for k, f in enumerate(S.FIELDS)}, "dist_t_q16": 2 ** 63 + 5}


# ---- the restatement against itself ----
@pytest.mark.parametrize("h,w", S.SHAPES)
@pytest.mark.parametrize("name", ["noisy", "disks", "truth_255", "corners", "mask_rule"])
def test_brute_force_distances_equal_the_distance_transform(name, h, w):
    """sqrt(d2) equals distance_transform_edt of the complement of the other surface to 1e-12"""
    u, t = S.case(name, h, w)
    m, t = S.mask_of(u), t != 0
    sm, st = S.surface(m), S.surface(t)
    dm, dt = S.distances(m, t)
    assert np.abs(np.sqrt(dm) - ndimage.distance_transform_edt(~st)[sm]).max() <= 1e-12
    assert np.abs(np.sqrt(dt) - ndimage.distance_transform_edt(~sm)[st]).max() <= 1e-12


def test_surface_is_the_four_neighbour_rule():
    rng = np.random.default_rng(4)
    s = rng.random((23, 37)) < 0.7
    p = np.pad(s, 1)
    inner = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    assert np.array_equal(S.surface(s), s & ~inner)
    full = np.ones((5, 7), bool)
    assert S.surface(full).sum() == 2 * 5 + 2 * 7 - 4                  # the border of a full plane is surface


@pytest.mark.parametrize("shift", [1, 2, 5])
def test_shifted_disks(shift):
    """two disks of radius r, centres `shift` columns apart: the extreme columns decide, hd2 == shift^2 both ways"""
    h, w, r = 64, 96, 20
    a, b = S.disk(h, w, 32, 40, r), S.disk(h, w, 32, 40 + shift, r)
    e = S.score(a, b, 4)
    assert e["hd2_m"] == e["hd2_t"] == shift * shift and e["defined"] == 1
    assert e["surf_m"] == e["surf_t"] and e["fp"] == e["fn"] > 0


def test_identical_masks_and_opposite_corners():
    for h, w in S.SHAPES:
        u, t = S.case("identical", h, w)
        e = S.score(S.mask_of(u), t != 0, 0)
        assert e["fp"] == e["fn"] == 0 and e["hd2_m"] == e["hd2_t"] == e["dist_m_q16"] == e["dist_t_q16"] == 0
        assert e["within_m"] == e["surf_m"] == e["within_t"] == e["surf_t"] > 0     # surface_dice == 1
        u, t = S.case("corners", h, w)
        e = S.score(S.mask_of(u), t != 0, 4)
        assert e["hd2_m"] == e["hd2_t"] == (h - 1) ** 2 + (w - 1) ** 2 and e["surf_m"] == e["surf_t"] == 1
        assert e["dist_m_q16"] == int(np.rint(np.sqrt(np.float64(e["hd2_m"])) * 65536))


def test_q16_rounds_half_to_even_and_is_exact_for_squares():
    d2 = np.array([0, 1, 4, 9, 2, 3, 65535 ** 2 + 1], dtype=np.int64)
    q = S.q16(d2)
    assert list(q[:4]) == [0, 65536, 2 * 65536, 3 * 65536] and q[4] == 92682 and q[5] == 113512
    assert q.dtype == np.uint64 and int(q[6]) < 2 ** 32


def test_the_mask_rule_of_the_restatement():
    u = np.array([np.nan, -0.0, 0.0, 1e-60, 1e-45, 2e-45, np.inf, -np.inf, -1e-60, 1.0])
    assert list(S.mask_of(u)) == [False, False, False, False, True, True, True, False, False, True]   # 1e-45 rounds to the smallest float
    assert list(S.mask_of(u, invert=True)) == [not v for v in S.mask_of(u)]
