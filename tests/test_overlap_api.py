"""CPU side of the component overlaps (include/chanvese_hip.h, "Component overlaps"): the boundary -- header, exports, the numpy dtype
against the C struct, what is refused before a device is touched --, cvh_match_overlaps (host arithmetic, no device) with == against
the brute force of overlap_util.py, and ObjectScore's figures."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import overlap_util as ou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
THRESHOLDS = [(1, 2), (2, 3), (19, 20), (1, 1)]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Component overlaps ----" in hdr
    assert re.search(r"typedef struct cvh_overlap \{ int32_t a, b; uint32_t count, pad; \} cvh_overlap;", hdr)
    assert re.search(r"typedef struct cvh_match \{ uint32_t objects_a, objects_b, tp, fp, fn, pad; \} cvh_match;", hdr)
    assert re.search(r"int cvh_overlaps\(cvh_context \*ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest,\s+"
                     r"const int32_t \*other /\* host \*/, cvh_overlap \*table, long cap, long \*pairs, int \*count\);", hdr)
    assert re.search(r"int cvh_overlaps_device\(cvh_context \*ctx, [^;]*const int32_t \*d_other, cvh_overlap \*table, long cap, long \*pairs, "
                     r"int \*count, void \*stream\);", hdr)
    assert re.search(r"int cvh_overlaps_device_batch\(cvh_context \*const \*ctxs, int n, [^;]*const int32_t \*const \*d_others, "
                     r"cvh_overlap \*const \*tables, const long \*caps, long \*pairs, int \*counts,\s+void \*stream\);", hdr)
    assert re.search(r"int cvh_match_overlaps\(const cvh_overlap \*table, long pairs, uint32_t num, uint32_t den, int32_t \*match_of_a, int k,\s+"
                     r"cvh_match \*out\);", hdr)
    for text in ("h w < 2^31, so a count fits 32 bits", "SORTED ON THE HOST", "Host waits: ONE for K, P and the overflow words",
                 "count den > num (area_a + area_b - count)", "0 < den <= 65535 and den <= 2 num <= 2 den", "NO ASSIGNMENT PROBLEM"):
        assert text in hdr, text
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in ("cvh_overlaps", "cvh_overlaps_device", "cvh_overlaps_device_batch", "cvh_match_overlaps"):
        assert hasattr(raw, name) and name in capi.EXPORTS
    assert hasattr(raw, "cvh_debug_overlap_launch_sets")


def test_struct_layouts_match_the_header(capi, tmp_path):
    """sizeof(cvh_overlap) == 16, and the numpy dtype and the ctypes struct agree with the C structs on every offset"""
    match_fields = [f for f, _ in capi.Match._fields_]
    src = tmp_path / "layout.c"
    body = '  printf("%zu", sizeof(cvh_overlap));\n' + "".join(f'  printf(" %zu", offsetof(cvh_overlap, {f}));\n' for f in capi.OVERLAP_DTYPE.names)
    body += '  printf("\\n%zu", sizeof(cvh_match));\n' + "".join(f'  printf(" %zu", offsetof(cvh_match, {f}));\n' for f in match_fields)
    src.write_text('#include "chanvese_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + body + '  printf("\\n");\n  return 0; }\n')
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines()
    dt = capi.OVERLAP_DTYPE
    assert [int(x) for x in lines[0].split()] == [16] + [dt.fields[f][1] for f in dt.names] == [16, 0, 4, 8, 12]
    assert dt.itemsize == 16 and dt == ou.OVERLAP_DTYPE
    assert [int(x) for x in lines[1].split()] == [ctypes.sizeof(capi.Match)] + [getattr(capi.Match, f).offset for f in match_fields]
    assert match_fields == ["objects_a", "objects_b", "tp", "fp", "fn", "pad"]


def test_refused_before_a_device_is_touched(capi):
    L = capi.lib()
    pairs, count = ctypes.c_long(7), ctypes.c_int(7)
    plane = np.zeros(4, np.int32)
    assert L.cvh_overlaps(None, 4, 0, 0, 0, 0, plane.ctypes.data, None, 0, ctypes.byref(pairs), ctypes.byref(count)) == ERR_ARG
    assert L.cvh_overlaps_device(None, 4, 0, 0, 0, 0, None, None, 0, ctypes.byref(pairs), ctypes.byref(count), None) == ERR_ARG
    assert L.cvh_overlaps_device_batch(None, 0, 4, 0, 0, 0, 0, None, None, None, None, None, None) == ERR_ARG
    assert b"cvh_overlaps_device_batch: empty member list" in L.cvh_last_error(None)
    arr = (ctypes.c_void_p * 1)(None)
    assert L.cvh_overlaps_device_batch(arr, 1, 4, 0, 0, 0, 0, None, None, None, None, None, None) == ERR_ARG
    assert b"member 0 is NULL" in L.cvh_last_error(None)
    assert (pairs.value, count.value) == (7, 7)


def random_table(rng):
    """a small table with heavy and light pairs: what two labelings of up to 6 objects and background can give"""
    na, nb = int(rng.integers(0, 6)), int(rng.integers(0, 6))
    bs = [0] + sorted(rng.choice(np.array([-5, -1, 3, 7, 100, 2 ** 31 - 1, -2 ** 31]), nb, replace=False).tolist())
    rows = []
    for a in range(na + 1):
        if a and rng.random() < 0.15:
            continue   # (a label without pixels cannot occur on the device, but the helper must cope)
        for b in sorted(bs):
            if rng.random() < 0.45:
                heavy = rng.random() < 0.4
                rows.append((a, b, int(rng.integers(50, 400)) if heavy else int(rng.integers(1, 12))))
    t = np.zeros(len(rows), ou.OVERLAP_DTYPE)
    for i, (a, b, c) in enumerate(rows):
        t[i] = (a, b, c, 0)
    return t


def call_match(capi, t, num, den, k=None, want_match=True):
    m = capi.Match()
    k = (int(t["a"].max()) if t.size else 0) if k is None else k
    match_of_a = np.full(max(k, 1), -77, np.int32)
    rc = capi.lib().cvh_match_overlaps(t.ctypes.data if t.size else None, t.size, num, den, match_of_a.ctypes.data if want_match else None, k,
                                       ctypes.byref(m))
    return rc, (m.objects_a, m.objects_b, m.tp, m.fp, m.fn), match_of_a[:k].tolist(), m.pad


def test_match_is_the_brute_force(capi):
    """a few hundred small random tables at 1/2, 2/3, 19/20 and 1/1: every count and every entry of match_of_a with =="""
    rng = np.random.default_rng(2024)
    matched = 0
    for _ in range(300):
        t = random_table(rng)
        for num, den in THRESHOLDS:
            want = ou.match(t, num, den)
            rc, got, match_of_a, pad = call_match(capi, t, num, den)
            assert rc == 0 and pad == 0
            assert got == want[:5], (t, num, den)
            assert match_of_a == want[5], (t, num, den)
            rc, got, _, _ = call_match(capi, t, num, den, want_match=False)
            assert rc == 0 and got == want[:5]
            matched += want[2]
        if t.size:
            score, py_match, ious = capi.match_overlaps(t, (2, 3))
            want = ou.match(t, 2, 3)
            assert (score.objects_a, score.objects_b, score.tp, score.fp, score.fn) == want[:5] and py_match.tolist() == want[5]
            assert score.tp_at == tuple(ou.match(t, q, 20)[2] for q in range(10, 20))
            assert len(ious) == score.tp and all(3 * n > 2 * d for _, _, n, d in ious)
    assert matched > 100   # (the tables do match now and then)


def test_ties_do_not_match(capi):
    """a of area 2 over b1 and b2 of area 1 by one pixel each: IoU exactly 1/2, so nothing matches at 1/2"""
    t = np.zeros(2, ou.OVERLAP_DTYPE)
    t["a"], t["b"], t["count"] = (1, 1), (1, 2), (1, 1)
    rc, got, match_of_a, _ = call_match(capi, t, 1, 2)
    assert rc == 0 and got == (1, 2, 0, 1, 2) and match_of_a == [0]
    same = np.zeros(2, ou.OVERLAP_DTYPE)   # an exact copy: IoU 1, above 19/20 and not above 1/1
    same["a"], same["b"], same["count"] = (0, 1), (0, -3), (5, 4)
    assert call_match(capi, same, 19, 20)[1:3] == ((1, 1, 1, 0, 0), [-3])
    assert call_match(capi, same, 1, 1)[1:3] == ((1, 1, 0, 1, 1), [0])
    rc, got, match_of_a, _ = call_match(capi, same[:0], 1, 2)   # the empty table
    assert rc == 0 and got == (0, 0, 0, 0, 0) and match_of_a == []


def test_match_refusals(capi):
    t = np.zeros(3, ou.OVERLAP_DTYPE)
    t["a"], t["b"], t["count"] = (0, 1, 2), (0, 4, -1), (3, 9, 2)
    assert call_match(capi, t, 1, 2)[0] == 0
    for num, den in ((1, 3), (49, 100), (1, 0), (0, 0), (40000, 65536), (3, 2), (0, 1)):
        assert call_match(capi, t, num, den)[0] == ERR_ARG, (num, den)
    assert call_match(capi, t, 65535, 65535)[0] == 0 and call_match(capi, t, 32768, 65535)[0] == 0
    assert call_match(capi, t[::-1].copy(), 1, 2)[0] == ERR_ARG          # unsorted
    twice = t[[0, 1, 1]].copy()
    assert call_match(capi, twice, 1, 2)[0] == ERR_ARG                   # a pair twice
    by_b = t.copy()
    by_b["a"], by_b["b"] = (1, 1, 1), (2 ** 31 - 1, 0, -1)               # b must ascend as a SIGNED integer
    assert call_match(capi, by_b, 1, 2)[0] == ERR_ARG
    by_b["b"] = (-2 ** 31, -1, 2 ** 31 - 1)
    assert call_match(capi, by_b, 1, 2)[0] == 0
    zero = t.copy()
    zero["count"][1] = 0
    assert call_match(capi, zero, 1, 2)[0] == ERR_ARG                    # a zero count
    assert call_match(capi, t, 1, 2, k=1)[0] == ERR_ARG                  # k too small for a = 2
    assert call_match(capi, t, 1, 2, k=1, want_match=False)[0] == 0      # ... which matters only with match_of_a
    assert call_match(capi, t, 1, 2, k=5)[2] == [4, -1, 0, 0, 0]         # the entries beyond the largest a are cleared
    m = capi.Match()
    assert capi.lib().cvh_match_overlaps(t.ctypes.data, 3, 1, 2, None, 0, None) == ERR_ARG
    assert capi.lib().cvh_match_overlaps(None, 3, 1, 2, None, 0, ctypes.byref(m)) == ERR_ARG
    assert capi.lib().cvh_match_overlaps(t.ctypes.data, -1, 1, 2, None, 0, ctypes.byref(m)) == ERR_ARG
    with pytest.raises(capi.CvhError):
        capi.match_overlaps(t, (1, 3))


def test_object_score_figures(capi):
    s = capi.ObjectScore(4, 5, 3, 1, 2, (3, 3, 3, 2, 2, 2, 1, 1, 0, 0))
    assert s.precision == 3 / 4 and s.recall == 3 / 5 and s.f1 == 6 / 9 and s.ap == 3 / 6
    assert s.mean_ap == sum(t / (9 - t) for t in s.tp_at) / 10
    none = capi.ObjectScore(0, 0, 0, 0, 0, (0,) * 10)
    for f in ("precision", "recall", "f1", "ap", "mean_ap"):
        assert math.isnan(getattr(none, f)), f
    no_truth = capi.ObjectScore(2, 0, 0, 2, 0, (0,) * 10)
    assert no_truth.precision == 0.0 and math.isnan(no_truth.recall) and no_truth.f1 == 0.0 and no_truth.ap == 0.0 and no_truth.mean_ap == 0.0
    no_objects = capi.ObjectScore(0, 3, 0, 0, 3, (0,) * 10)
    assert math.isnan(no_objects.precision) and no_objects.recall == 0.0
    assert math.isnan(capi.ObjectScore(1, 1, 1, 0, 0).mean_ap)   # (without the ten thresholds)
