"""numpy restatement of the header's "Component overlaps" (include/chanvese_hip.h): the label plane A from components_util's labelling and
cleaning (no scipy shortcut for the numbering), the contingency table by np.unique on the pairs plus np.lexsort, and a brute-force match
over ALL pairs in Python integers.  It is the checker of tests/test_overlap_restatement.py (which holds it against a double loop),
tests/test_overlap_api.py, tests/test_gpu_overlap.py, tests/test_gpu_torch_overlap.py and tests/test_cli_overlap.py."""
import numpy as np

import components_util as cu

OVERLAP_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("count", np.uint32), ("pad", np.uint32)])


def labels_of(mask, conn=4, min_area=0, fill_holes=0, keep_largest=False):
    """(A, K): the labels of the cleaned mask, 0 background, 1 .. K numbered by smallest flat index after cleaning"""
    m = np.asarray(mask).astype(bool)
    if min_area > 1 or fill_holes or keep_largest:
        m = cu.clean(m, conn, min_area, fill_holes, keep_largest).astype(bool)
    lab, comp = cu.label(m, conn, boxes=False)
    return lab.astype(np.int32), int(comp.size)


def table_of(A, B):
    """the rows of two label planes: np.unique on the pairs, then the header's order (a ascending, then b ascending, signed)"""
    A, B = np.asarray(A, np.int32).reshape(-1), np.asarray(B, np.int32).reshape(-1)
    assert A.shape == B.shape
    pairs, counts = np.unique(np.stack([A, B], axis=1), axis=0, return_counts=True)
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    t = np.zeros(order.size, OVERLAP_DTYPE)
    t["a"], t["b"], t["count"] = pairs[order, 0], pairs[order, 1], counts[order]
    return t


def overlaps(mask, other, conn=4, min_area=0, fill_holes=0, keep_largest=False):
    """(rows, K) of cvh_overlaps for a boolean mask (cvh_get_mask's, invert applied) and the plane B"""
    A, K = labels_of(mask, conn, min_area, fill_holes, keep_largest)
    return table_of(A, other), K


def match(rows, num, den):
    """(objects_a, objects_b, tp, fp, fn, match_of_a) by brute force: every (a != 0, b != 0) pair of objects, present in the table or
    not, with count den > num (area_a + area_b - count) in Python integers; match_of_a has max(a) entries and keeps the LAST b that
    matched (for a threshold >= 1/2 there is at most one)."""
    rows = [(int(r["a"]), int(r["b"]), int(r["count"])) for r in rows]
    area_a, area_b, count = {}, {}, {}
    for a, b, c in rows:
        area_a[a] = area_a.get(a, 0) + c
        area_b[b] = area_b.get(b, 0) + c
        count[(a, b)] = c
    objs_a, objs_b = sorted(a for a in area_a if a != 0), sorted(b for b in area_b if b != 0)
    match_of_a = [0] * max([a for a, _, _ in rows] + [0])
    tp = 0
    for a in objs_a:
        for b in objs_b:
            c = count.get((a, b), 0)
            if c * den > num * (area_a[a] + area_b[b] - c):
                tp += 1
                match_of_a[a - 1] = b
    return len(objs_a), len(objs_b), tp, len(objs_a) - tp, len(objs_b) - tp, match_of_a


def grid_labels(h, w, cell=32):
    """a truth plane of cell x cell squares with distinct labels 1 .. (row-major)"""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((yy // cell) * ((w + cell - 1) // cell) + xx // cell + 1).astype(np.int32)


def assert_rows_equal(got, want, what=""):
    assert got.dtype == want.dtype == OVERLAP_DTYPE, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (what, got[:6], want[:6])
