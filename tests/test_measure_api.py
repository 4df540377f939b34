"""CPU side of the component measures (include/chanvese_hip.h, "Component measures"): the boundary -- header, exports, the numpy dtype
against the C struct, what is refused before a device is touched --, cvh_region_shape_of (host arithmetic, no device) against its Python
restatement, and the restatement of the table (measure_util.py) against a brute force that shares nothing with it."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import components_util as cu
import measure_util as mu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Component measures ----" in hdr
    assert re.search(r"int cvh_measure\(cvh_context \*ctx, int conn, int invert, long min_area, long fill_holes, int keep_largest,\s+"
                     r"cvh_region \*table, int cap, int \*count, void \*stream\);", hdr)
    assert re.search(r"int cvh_measure_batch\(cvh_context \*const \*ctxs, int n, int conn, int invert, long min_area, long fill_holes, "
                     r"int keep_largest,\s+cvh_region \*const \*tables, const int \*caps, int \*counts, void \*stream\);", hdr)
    assert re.search(r"int cvh_region_shape_of\(const cvh_region \*r, int channels, cvh_region_shape \*out\);", hdr)
    for text in ("h <= 65535, w <= 65535 and h w < 2^31", "2^63", "ONE for the counts, and a SECOND where any rows are asked for",
                 "theta = 0.5 atan2(2 mu11, mu20 - mu02)"):
        assert text in hdr, text
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in ("cvh_measure", "cvh_measure_batch", "cvh_region_shape_of"):
        assert hasattr(raw, name) and name in capi.EXPORTS


def test_struct_layouts_match_the_header(capi, tmp_path):
    """sizeof(cvh_region) == 128, and the numpy dtypes agree with the C structs on every offset"""
    cases = (("cvh_region", capi.REGION_DTYPE, 128), ("cvh_region_shape", capi.REGION_SHAPE_DTYPE, 112))
    src = tmp_path / "layout.c"
    body = ""
    for struct, dt, _ in cases:
        body += f'  printf("%zu", sizeof({struct}));\n' + "".join(f'  printf(" %zu", offsetof({struct}, {f}));\n' for f in dt.names) + '  printf("\\n");\n'
    src.write_text('#include "chanvese_hip.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + body + "  return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.splitlines()
    for (struct, dt, size), line in zip(cases, lines):
        assert [int(x) for x in line.split()] == [dt.itemsize] + [dt.fields[f][1] for f in dt.names], struct
        assert dt.itemsize == size
    assert capi.REGION_DTYPE == mu.REGION_DTYPE
    assert capi.REGION_DTYPE.names[:6] == capi.COMPONENT_DTYPE.names   # "exactly cvh_component's fields"


def test_refused_before_a_device_is_touched(capi):
    L = capi.lib()
    count = ctypes.c_int(7)
    assert L.cvh_measure(None, 4, 0, 0, 0, 0, None, 0, ctypes.byref(count), None) == ERR_ARG
    assert L.cvh_measure_batch(None, 0, 4, 0, 0, 0, 0, None, None, None, None) == ERR_ARG
    assert b"cvh_measure_batch: empty member list" in L.cvh_last_error(None)
    arr = (ctypes.c_void_p * 1)(None)
    assert L.cvh_measure_batch(arr, 1, 4, 0, 0, 0, 0, None, None, None, None) == ERR_ARG
    assert b"member 0 is NULL" in L.cvh_last_error(None)
    row, out = np.zeros(1, capi.REGION_DTYPE), np.zeros(1, capi.REGION_SHAPE_DTYPE)
    assert L.cvh_region_shape_of(row.ctypes.data, 1, out.ctypes.data) == ERR_ARG   # area == 0
    row["area"] = 1
    assert L.cvh_region_shape_of(row.ctypes.data, 1, out.ctypes.data) == 0
    assert L.cvh_region_shape_of(row.ctypes.data, 2, out.ctypes.data) == ERR_ARG
    assert L.cvh_region_shape_of(row.ctypes.data, 0, out.ctypes.data) == ERR_ARG
    assert L.cvh_region_shape_of(None, 1, out.ctypes.data) == ERR_ARG
    assert L.cvh_region_shape_of(row.ctypes.data, 1, None) == ERR_ARG
    with pytest.raises(capi.CvhError):
        capi.region_shapes(np.zeros(2, capi.REGION_DTYPE), 1)


def planes_for(h, w, channels, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(channels)]


MASKS = [("rand50", 9, 13), ("rand50", 1, 40), ("rand50", 40, 1), ("spiral", 12, 17), ("comb", 7, 9), ("rings", 16, 16), ("isolated", 6, 7),
         ("inside", 5, 8), ("outside", 4, 4), ("diagonal", 8, 8)]


def small_mask(kind, h, w):
    if kind == "rand50":
        return np.random.default_rng(h * 131 + w).random((h, w)) < 0.5
    if kind == "inside":
        return np.ones((h, w), bool)
    if kind == "outside":
        return np.zeros((h, w), bool)
    return getattr(cu, kind)(h, w)


@pytest.mark.parametrize("kind,h,w", MASKS)
@pytest.mark.parametrize("conn", [4, 8])
def test_restatement_against_brute_force(kind, h, w, conn):
    """a Python loop per label: np.nonzero on lab == k for the sums, a loop per pixel and edge for perimeter and border"""
    m = small_mask(kind, h, w)
    channels = 3 if (h + w) % 2 else 1
    planes = planes_for(h, w, channels, h + 7 * w)
    t = mu.measure(m, planes, conn)
    lab, comp = cu.label(m, conn)
    assert t.size == comp.size == int(lab.max())
    for k in range(1, t.size + 1):
        row = t[k - 1]
        rr, cc = np.nonzero(lab == k)
        rr, cc = [int(v) for v in rr], [int(v) for v in cc]
        assert int(row["first"]) == min(r * w + c for r, c in zip(rr, cc))
        assert int(row["area"]) == len(rr)
        assert (int(row["x0"]), int(row["y0"]), int(row["x1"]), int(row["y1"])) == (min(cc), min(rr), max(cc), max(rr))
        assert int(row["sx"]) == sum(cc) and int(row["sy"]) == sum(rr)
        assert int(row["sxx"]) == sum(c * c for c in cc) and int(row["syy"]) == sum(r * r for r in rr)
        assert int(row["sxy"]) == sum(r * c for r, c in zip(rr, cc))
        for j in range(3):
            vals = [int(planes[j][r, c]) for r, c in zip(rr, cc)] if j < channels else []
            assert int(row["s1"][j]) == sum(vals) and int(row["s2"][j]) == sum(v * v for v in vals)
        perimeter = border = 0
        for r, c in zip(rr, cc):
            border += r in (0, h - 1) or c in (0, w - 1)
            for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                y, x = r + dr, c + dc
                outside = not (0 <= y < h and 0 <= x < w)
                perimeter += outside or not m[y, x]
                assert outside or not m[y, x] or lab[y, x] == k   # a foreground 4-neighbour is of the same component
        assert int(row["perimeter"]) == perimeter and int(row["border"]) == border and int(row["reserved"]) == 0
        assert np.isclose(mu.shape_of(row, channels)["cx"], np.mean(cc)) and np.isclose(mu.shape_of(row, channels)["cy"], np.mean(rr))
        assert np.isclose(mu.shape_of(row, channels)["mu20"], np.var(cc), atol=1e-9)
        for j in range(channels):
            assert np.isclose(mu.shape_of(row, channels)["var"][j], np.var(planes[j][lab == k].astype(float)), atol=1e-7)


def hand_rows(capi):
    """rows whose sums sit near the top of the 64-bit range: A sxx - sx^2 needs more than 64 bits, and its conversion rounds"""
    rows = np.zeros(6, capi.REGION_DTYPE)
    # a 32768 x 65535 plane wholly inside: the header's bounds at their edge
    h, w = 32768, 65535
    A = h * w
    rows[0]["area"] = A
    rows[0]["sx"] = h * (w * (w - 1) // 2)
    rows[0]["sy"] = w * (h * (h - 1) // 2)
    rows[0]["sxx"] = h * ((w - 1) * w * (2 * w - 1) // 6)
    rows[0]["syy"] = w * ((h - 1) * h * (2 * h - 1) // 6)
    rows[0]["sxy"] = (w * (w - 1) // 2) * (h * (h - 1) // 2)
    rows[0]["s1"] = (A * 255, A * 3, 12345)
    rows[0]["s2"] = (A * 255 * 255, A * 11, 2 ** 40 + 1)
    # sums near 2^62 with odd low bits: every numerator is a difference of two products beyond 2^64
    rows[1]["area"] = 2 ** 31 - 1
    for f, v in (("sx", 2 ** 46 + 12345), ("sy", 2 ** 45 + 999), ("sxx", 2 ** 62 + 2 ** 31 + 7), ("syy", 2 ** 62 - 2 ** 20 - 3), ("sxy", 2 ** 61 + 5)):
        rows[1][f] = v
    rows[1]["s1"] = (2 ** 38 + 1, 2 ** 37 + 3, 2 ** 36 + 5)
    rows[1]["s2"] = (2 ** 46 + 2 ** 15 + 1, 2 ** 46 - 1, 2 ** 45 + 77)
    # a negative mu11 beyond 64 bits, and a negative "variance" (not a moment of any plane: the helper must not assume the sign)
    rows[2] = rows[1]
    rows[2]["sxy"] = 2 ** 55 + 1
    rows[2]["s2"] = (1, 2, 3)
    # a tie of the rounding: numerator 2^70 + 2^17 rounds to even (down), 2^70 + 3 2^17 up
    rows[3]["area"] = 2 ** 16
    rows[3]["sxx"] = 2 ** 54 + 2
    rows[3]["syy"] = 2 ** 54 + 6
    rows[3]["sx"] = 0
    rows[3]["sxy"] = 2 ** 54 + 3
    rows[3]["sy"] = 2 ** 9
    # one pixel, and a horizontal line (minor axis 0)
    rows[4]["area"], rows[4]["sx"], rows[4]["sy"], rows[4]["sxx"], rows[4]["syy"], rows[4]["sxy"] = 1, 65534, 3, 65534 ** 2, 9, 3 * 65534
    rows[4]["s1"], rows[4]["s2"] = (255, 0, 7), (65025, 0, 49)
    n = 1000
    rows[5]["area"], rows[5]["sx"], rows[5]["sy"] = n, n * (n - 1) // 2, 5 * n
    rows[5]["sxx"], rows[5]["syy"], rows[5]["sxy"] = (n - 1) * n * (2 * n - 1) // 6, 25 * n, 5 * (n * (n - 1) // 2)
    return rows


@pytest.mark.parametrize("channels", [1, 3])
def test_shape_helper_against_the_restatement(capi, channels):
    """== up to var (a 64-bit intermediate in the C helper fails on the hand-built rows), rel 1e-12 behind libm"""
    rows = hand_rows(capi)
    A, sxx, sx = int(rows[1]["area"]), int(rows[1]["sxx"]), int(rows[1]["sx"])
    assert A * sxx - sx * sx > 2 ** 90 and (A * sxx) % 2 ** 64 != A * sxx
    got = capi.region_shapes(rows, channels)
    mu.assert_shapes_match(got, rows, channels)
    assert got["mu11"][2] < 0 and got["var"][2][0] < 0
    assert got["minor"][5] == 0.0 or got["minor"][5] < 1e-6
    assert got["mu20"][4] == 0.0 and got["cx"][4] == 65534.0
    if channels == 1:
        assert not got["mean"][:, 1:].any() and not got["var"][:, 1:].any()
    # and on the rows of real masks
    for kind, h, w in MASKS:
        t = mu.measure(small_mask(kind, h, w), planes_for(h, w, channels, 3), 8)
        mu.assert_shapes_match(capi.region_shapes(t, channels), t, channels)
