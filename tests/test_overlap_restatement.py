"""The restatement of the header's "Component overlaps" (overlap_util.py) against a double loop that shares nothing with it, on planes up to
12 x 12: the rows and their order, counts that add up to h w, and areas that equal the component table's.  No library, no device."""
import numpy as np
import pytest

import components_util as cu
import overlap_util as ou

CASES = [(1, 1), (1, 12), (12, 1), (3, 5), (7, 9), (12, 12), (11, 12)]
EXTREMES = np.array([-1, -2 ** 31, 2 ** 31 - 1, 0, 5], np.int64)


def planes(h, w, seed):
    rng = np.random.default_rng(seed)
    mask = rng.random((h, w)) < 0.55
    other = EXTREMES[rng.integers(0, EXTREMES.size, (h, w))].astype(np.int32)
    return mask, other


def double_loop(A, B):
    """a dictionary filled pixel by pixel, its keys sorted as Python tuples of signed integers"""
    count = {}
    for r in range(A.shape[0]):
        for c in range(A.shape[1]):
            key = (int(A[r, c]), int(B[r, c]))
            count[key] = count.get(key, 0) + 1
    return [(a, b, n) for (a, b), n in sorted(count.items())]


@pytest.mark.parametrize("h,w", CASES)
@pytest.mark.parametrize("conn", [4, 8])
def test_table_against_a_double_loop(h, w, conn):
    for seed in range(4):
        mask, other = planes(h, w, 100 * h + w + seed)
        for clean in ((0, 0, False), (3, 0, False), (0, -1, False), (2, 2, True)):
            rows, K = ou.overlaps(mask, other, conn, *clean)
            A, K2 = ou.labels_of(mask, conn, *clean)
            assert K == K2 == int(A.max())
            assert np.array_equal(A != 0, cu.clean(mask, conn, *clean).astype(bool) if any(clean) else mask)
            want = double_loop(A, other)
            assert [(int(r["a"]), int(r["b"]), int(r["count"])) for r in rows] == want
            assert not rows["pad"].any() and rows.dtype.itemsize == 16
            assert int(rows["count"].astype(np.int64).sum()) == h * w


@pytest.mark.parametrize("h,w", CASES)
def test_areas_are_the_component_table_s(h, w):
    mask, other = planes(h, w, 7 * h + w)
    for conn in (4, 8):
        rows, K = ou.overlaps(mask, other, conn)
        _, comp = cu.label(mask, conn)
        assert K == comp.size
        for k in range(1, K + 1):
            assert int(rows["count"][rows["a"] == k].sum()) == int(comp["area"][k - 1])
        assert int(rows["count"][rows["a"] == 0].sum()) == int((~mask).sum())


def test_numbering_follows_the_cleaning():
    """a speck in front of a blob: with min_area the blob becomes label 1"""
    mask = np.zeros((6, 8), bool)
    mask[0, 0] = True
    mask[2:5, 2:6] = True
    other = np.arange(48, dtype=np.int32).reshape(6, 8)
    raw, k_raw = ou.overlaps(mask, other)
    cleaned, k_clean = ou.overlaps(mask, other, 4, 2)
    assert (k_raw, k_clean) == (2, 1)
    assert int(raw["count"][raw["a"] == 2].sum()) == 12 and int(cleaned["count"][cleaned["a"] == 1].sum()) == 12
    assert raw.size == cleaned.size == 48 and int(cleaned["a"][cleaned["b"] == 0][0]) == 0


def test_signed_order():
    A = np.array([[1, 1, 1, 1, 0]], np.int32)
    B = np.array([[2 ** 31 - 1, -1, 0, -2 ** 31, -7]], np.int32)
    t = ou.table_of(A, B)
    assert [(int(r["a"]), int(r["b"])) for r in t] == [(0, -7), (1, -2 ** 31), (1, -1), (1, 0), (1, 2 ** 31 - 1)]


def test_brute_force_match_on_a_hand_case():
    """a of area 2 over b1 and b2 of area 1: IoU 1/2 each, nothing matches at 1/2; an exact copy matches up to 1/1 excluded"""
    rows = np.zeros(2, ou.OVERLAP_DTYPE)
    rows["a"], rows["b"], rows["count"] = (1, 1), (1, 2), (1, 1)
    assert ou.match(rows, 1, 2) == (1, 2, 0, 1, 2, [0])
    same = np.zeros(2, ou.OVERLAP_DTYPE)
    same["a"], same["b"], same["count"] = (0, 1), (0, 9), (5, 4)
    assert ou.match(same, 19, 20) == (1, 1, 1, 0, 0, [9])
    assert ou.match(same, 1, 1) == (1, 1, 0, 1, 1, [0])
