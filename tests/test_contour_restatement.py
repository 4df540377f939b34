"""The restatement of "Contours" (tests/contour_util.py) against properties that do not reuse its code (CPU): the loops filled back by the
even-odd rule along pixel rows give the mask; the area2 add up to twice the area; loops = components + holes by the components
restatement; corner loops have an even point count >= 4; the 2 x 2 diagonal."""
import numpy as np
import pytest

import components_util as cu
import contour_util as ct

MASKS = dict(ct.small_masks(), noise=ct.noise(48, 80), spiral=cu.spiral(21, 30), rings=cu.rings(17, 23))


def fill(loops, points, h, w):
    """even-odd along pixel rows: a pixel is inside where an odd number of vertical polygon sides lies to its left"""
    cross = np.zeros((h, w + 1), np.int64)
    for l in loops:
        p = points[int(l["offset"]):int(l["offset"]) + int(l["points"])]
        for (x0, y0), (x1, y1) in zip(p, np.roll(p, -1, axis=0)):
            if x0 == x1:
                cross[min(y0, y1):max(y0, y1), x0] += 1
            else:
                assert y0 == y1
    return (np.cumsum(cross, axis=1)[:, :w] % 2) == 1


@pytest.mark.parametrize("name", sorted(MASKS))
@pytest.mark.parametrize("conn", [4, 8])
def test_properties(name, conn):
    m = MASKS[name]
    h, w = m.shape
    for simplify in (False, True):
        loops, points = ct.trace(m, conn, simplify)
        assert np.array_equal(fill(loops, points, h, w), m)
        assert int(loops["area2"].sum()) == 2 * int(m.sum())
        assert int(loops["points"].sum()) == points.shape[0]
        assert np.array_equal(loops["offset"], (np.cumsum(loops["points"], dtype=np.uint64) - loops["points"]).astype(np.uint64))
        assert np.all(np.diff(loops["first"].astype(np.int64)) > 0)
        if simplify:
            assert np.all(loops["points"] % 2 == 0) and np.all(loops["points"] >= 4)
        else:
            assert np.array_equal(loops["points"], loops["edges"])
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = m
    k_fg = cu.label(m, conn, False)[1].size
    k_bg = cu.label(~pad, 8 if conn == 4 else 4, False)[1].size   # the outside is one of them
    assert loops.size == k_fg + k_bg - 1
    assert int((loops["area2"] > 0).sum()) == k_fg and int((loops["area2"] < 0).sum()) == k_bg - 1


def test_two_by_two_diagonal():
    for m in (ct.small_masks()["2x2_diagonal"], ct.small_masks()["2x2_antidiagonal"]):
        l8, _ = ct.trace(m, 8)
        l4, _ = ct.trace(m, 4)
        assert l8["edges"].tolist() == [8] and l4["edges"].tolist() == [4, 4]


def test_single_pixel_by_hand():
    loops, points = ct.trace(np.ones((1, 1), bool), 8, True)
    assert loops.tolist() == [(0, 4, 4, 0, 0, 2)]
    assert points.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]]
