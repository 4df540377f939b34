"""CPU side of "Object split" (include/chanvese_hip.h): the two restatements of split_util.py against each other, the properties the
header states -- the unchanged cases, the pieces behind the cut, the fixpoint under a random order of relaxation -- and the demonstration
scene held to its integers.  Nothing here touches the library."""
import numpy as np
import pytest
from scipy import ndimage

import components_util as CU
import split_util as S

SHAPES = S.SMALL_SHAPES + [(33, 65)]


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("name", list(S.CASES))
def test_the_two_restatements_agree(name, conn):
    for h, w in SHAPES:
        f0 = S.start_set(S.case(name, h, w), conn)
        for r2 in S.R2S:
            a = S.expected(name, h, w, conn, r2)
            lab, k = S.split_queue(f0, conn, r2)
            assert k == a.K and np.array_equal(lab, a.labels), (name, (h, w), conn, r2)
            assert ((a.labels > 0) == f0).all() and a.table["area"].sum() == f0.sum()


@pytest.mark.parametrize("conn", (4, 8))
def test_r2_zero_and_everything_eroded_are_the_components_of_the_clean_mask(conn):
    for name, shape in (("demo", (64, 64)), ("touching", (33, 64)), ("all_inside", (9, 21)), ("all_outside", (9, 21))):
        f0 = S.start_set(S.case(name, *shape), conn)
        want, k = ndimage.label(f0, S._structure(conn))
        lab_cu, tab_cu = CU.label(f0, conn)
        for r2 in (0, 2 ** 32 - 1):
            a = S.expected(name, *shape, conn, r2)
            assert a.K == k and np.array_equal(a.labels, want) and np.array_equal(a.labels, lab_cu), (name, conn, r2)
            assert np.array_equal(a.table, tab_cu), (name, conn, r2)
            if conn == 8 or name != "touching":   # (4-components that touch diagonally are held apart: the header says so)
                assert not a.cut.any(), (name, conn, r2)


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("name", ("touching", "demo", "noisy"))
def test_behind_the_cut_every_piece_lies_inside_one_label(name, conn):
    for h, w in ((33, 64), (64, 64)):
        for r2 in (1, 4, 9, 25, 81):
            a = S.expected(name, h, w, conn, r2)
            pieces, k = ndimage.label(a.pieces, np.ones((3, 3), bool))   # 8-components: the coarser of the two
            for n in range(1, k + 1):
                assert np.unique(a.labels[pieces == n]).size == 1, (name, (h, w), conn, r2, n)
            both = a.labels.astype(np.int64) * a.pieces
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q = S.shifted(both, dy, dx, 0)
                    assert not ((both > 0) & (q > 0) & (q != both)).any()   # no two pixels of different labels are 8-adjacent


@pytest.mark.parametrize("seed", (0, 1, 2))
@pytest.mark.parametrize("conn", (4, 8))
def test_a_random_relaxation_order_reaches_the_same_keys(conn, seed):
    for name, shape, r2 in (("touching", (33, 40), 9), ("demo", (64, 64), 64), ("noisy", (9, 21), 1)):
        f0 = S.start_set(S.case(name, *shape), conn)
        got, sync = S.relax_random(f0, conn, r2, seed)
        assert np.array_equal(got, sync), (name, conn, r2)


def sizes(a):
    return np.bincount(a.labels.ravel(), minlength=a.K + 1)[1:].tolist()


def test_the_demonstration():
    """two disks of radius 12 that overlap, a 3 x 3 square and a bar, conn = 4: labels in raster order of the markers are the square, the
    blob's cores, the bar"""
    d = S.demonstration()
    assert d.sum() == 829 + 9 + 60
    a = S.Split(d, 4, 81)
    assert (a.K, sizes(a), int(a.cut.sum())) == (4, [9, 423, 406, 60], 19)
    a = S.Split(d, 4, 100)
    assert (a.K, sizes(a), int(a.cut.sum())) == (4, [9, 416, 413, 60], 19)
    a = S.Split(d, 4, 49)
    assert (a.K, sizes(a), int(a.cut.sum())) == (3, [9, 829, 60], 0)
    a = S.Split(d, 4, 150)
    assert (a.K, sizes(a), int(a.cut.sum())) == (3, [9, 829, 60], 0) and not a.eroded.any()
    a = S.Split(d, 4, 64)                     # the method's sensitivity to the radius: a spurious third object of 37 pixels
    assert a.K == 5 and sorted(sizes(a)) == sorted([9, 396, 396, 37, 60])
    for r2 in (81, 100, 49, 150, 64):
        assert np.array_equal(S.split_queue(d, 4, r2)[0], S.Split(d, 4, r2).labels)


def test_the_spiral_is_one_corridor_with_one_marker():
    m, centre = S.spiral(64, 128)
    a = S.Split(m, 4, 1)
    assert a.K == 1 and a.markers[centre] and a.markers.sum() == 2 and a.rounds > 2000   # (the block's pixel beside the corridor survives too)
    assert all(m[31:33, c].all() for c in range(70, 128, 2) if m[31, c]) and m[:, 63:65].all(axis=1).sum() >= 20   # it crosses both seams, often
