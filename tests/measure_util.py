"""numpy restatement of the header's "Component measures" (include/chanvese_hip.h): the rows of cvh_measure from a boolean mask and the
image planes, built on components_util.label / clean, and cvh_region_shape_of's formulas in Python integers and floats.  It is the checker
of tests/test_measure_api.py (which holds it against a brute force), tests/test_gpu_measure.py and tests/test_cli_measure.py."""
import math

import numpy as np

import components_util as cu

REGION_DTYPE = np.dtype([("first", np.uint32), ("area", np.uint32), ("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32),
                         ("border", np.uint32), ("reserved", np.uint32)] +
                        [(f, np.uint64) for f in ("perimeter", "sx", "sy", "sxx", "syy", "sxy")] + [("s1", np.uint64, 3), ("s2", np.uint64, 3)])
INT_FIELDS = ("first", "area", "x0", "y0", "x1", "y1", "border", "reserved", "perimeter", "sx", "sy", "sxx", "syy", "sxy", "s1", "s2")
EXACT_SHAPE_FIELDS = ("cx", "cy", "mu20", "mu02", "mu11", "mean", "var")
LIBM_SHAPE_FIELDS = ("theta", "major", "minor")


def _sum_by(k, values, size):
    out = np.zeros(size, np.uint64)
    np.add.at(out, k, values.astype(np.uint64))   # exact: integers all the way
    return out


def measure(mask, planes, conn=4):
    """The table of cvh_measure for a boolean mask (already cleaned, if it is to be) and the list of uint8 planes."""
    m = np.asarray(mask).astype(bool)
    h, w = m.shape
    lab, comp = cu.label(m, conn)
    t = np.zeros(comp.size, REGION_DTYPE)
    for f in comp.dtype.names:
        t[f] = comp[f]
    if not comp.size:
        return t
    r, c = np.nonzero(m)
    k = lab[r, c] - 1
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = m
    fg_neighbours = pad[:-2, 1:-1].astype(np.int64) + pad[2:, 1:-1] + pad[1:-1, :-2] + pad[1:-1, 2:]
    t["perimeter"] = _sum_by(k, 4 - fg_neighbours[r, c], comp.size)
    t["border"] = _sum_by(k, (r == 0) | (r == h - 1) | (c == 0) | (c == w - 1), comp.size)
    r64, c64 = r.astype(np.uint64), c.astype(np.uint64)
    for name, v in (("sx", c64), ("sy", r64), ("sxx", c64 * c64), ("syy", r64 * r64), ("sxy", r64 * c64)):
        t[name] = _sum_by(k, v, comp.size)
    for j, p in enumerate(planes):
        v = np.asarray(p)[r, c].astype(np.uint64)
        t["s1"][:, j] = _sum_by(k, v, comp.size)
        t["s2"][:, j] = _sum_by(k, v * v, comp.size)
    return t


def measure_clean(mask, planes, conn=4, min_area=0, fill_holes=0, keep_largest=False):
    return measure(cu.clean(mask, conn, min_area, fill_holes, keep_largest), planes, conn)


def shape_of(row, channels):
    """cvh_region_shape_of: exact integers, ONE float(int) per numerator (round to nearest even), then IEEE operations."""
    A = int(row["area"])
    sx, sy, sxx, syy, sxy = (int(row[f]) for f in ("sx", "sy", "sxx", "syy", "sxy"))
    a = float(A)
    a2 = a * a
    out = {"cx": float(sx) / a, "cy": float(sy) / a,
           "mu20": float(A * sxx - sx * sx) / a2, "mu02": float(A * syy - sy * sy) / a2, "mu11": float(A * sxy - sx * sy) / a2,
           "mean": [0.0] * 3, "var": [0.0] * 3}
    for j in range(channels):
        s1, s2 = int(row["s1"][j]), int(row["s2"][j])
        out["mean"][j] = float(s1) / a
        out["var"][j] = float(A * s2 - s1 * s1) / a2
    half, mid = (out["mu20"] - out["mu02"]) / 2, (out["mu20"] + out["mu02"]) / 2
    root = math.sqrt(half * half + out["mu11"] * out["mu11"])
    l1, l2 = mid + root, mid - root
    out["theta"] = 0.5 * math.atan2(2 * out["mu11"], out["mu20"] - out["mu02"])
    out["major"] = 4 * math.sqrt(l1)
    out["minor"] = 0.0 if l2 < 0 else 4 * math.sqrt(l2)
    return out


def assert_tables_equal(got, want, what=""):
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in INT_FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, got[f][:4], want[f][:4])


def assert_shapes_match(got, table, channels, rel=1e-12):
    """got: capi.region_shapes(table, channels).  == up to var, rel for the three fields behind libm."""
    for i in range(table.size):
        want = shape_of(table[i], channels)
        for f in EXACT_SHAPE_FIELDS:
            g = got[f][i].tolist()
            assert g == want[f], (i, f, g, want[f])
        for f in LIBM_SHAPE_FIELDS:
            g = float(got[f][i])
            assert abs(g - want[f]) <= rel * abs(want[f]), (i, f, g, want[f])
