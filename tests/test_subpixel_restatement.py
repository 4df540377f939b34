"""The restatements of "Subpixel contours" (subpixel_util) against each other and against the analytic disk: no device.  The traced one
(the loops of contour_util, numpy FP64) and the direct one (all foreground / neighbour pairs, Python floats, no tracing) must give the
same points; the disk's figures are the issue's, computed from the header's definition."""
import math

import numpy as np
import pytest

import contour_util as ct
import subpixel_util as su

SMALL = ct.small_masks()
COMBOS = [(conn, invert) for conn in (4, 8) for invert in (False, True)]


@pytest.mark.parametrize("name", sorted(SMALL))
def test_the_two_restatements_agree_on_the_small_masks(name):
    u = su.from_mask(SMALL[name], seed=len(name))
    for conn, invert in COMBOS:
        loops, pts = su.check_against_direct(u, conn, invert)
        assert loops.tobytes() == ct.trace(SMALL[name] != invert, conn, False)[0].tobytes()
        assert pts.dtype == np.float64 and pts.shape == (int(loops["edges"].sum()), 2)


def test_the_two_restatements_agree_on_ring_and_blob_and_cleaned_noise():
    for conn, invert in COMBOS:
        su.check_against_direct(su.from_mask(ct.ring_and_blob(), 2), conn, invert)
        loops, pts = su.check_against_direct(su.from_mask(ct.noise(), 3), conn, invert, 5, -1, True)
        assert loops.size >= 1 and pts.shape[0] >= 4


def test_special_values_fall_back_to_the_midpoint():
    u = su.special()
    for state32 in (False, True):
        for conn, invert in COMBOS:
            loops, pts = su.check_against_direct(u, conn, invert, state32=state32)
            assert np.all(np.isfinite(pts)) and loops.size >= 1
    # the overflowing pair of row 5: columns 20 | 21 are +1e308 | -1e308, the edge between them sits at its midpoint
    _, pts, ids = su.trace_subpixel_edges(u, 8)
    at = ids.tolist().index(4 * (5 * u.shape[1] + 20) + 1)
    assert pts[at].tolist() == [21.0, 5.5]
    # the edge of row 6 between 1.0 (column 23) and 0.0 (column 24): b = 0 puts the point on the neighbour's centre, t = 1
    assert pts[ids.tolist().index(4 * (6 * u.shape[1] + 23) + 1)].tolist() == [24.5, 6.5]
    # a filled hole leaves no edge behind: the one loop is the outer boundary
    m = np.ones((9, 9), bool)
    m[4, 4] = False
    m[0, :] = False
    loops, pts = su.check_against_direct(su.from_mask(m, 5), 4, False, 0, -1, False)
    assert loops.size == 1 and pts.shape[0] == 2 * (8 + 9)


def test_disk_64_subpixel_points_lie_on_the_circle_and_midpoints_do_not():
    """restatement: 162 edges, 0.0056 px against 0.499 px"""
    u = su.disk(64)
    for conn in (4, 8):
        loops, pts = su.check_against_direct(u, conn, False)
        sub, mid = su.radial_error(pts), su.radial_error(su.midpoints(u, conn))
        print(f"conn {conn}: {pts.shape[0]} edges, subpixel {sub:.4f} px, midpoints {mid:.4f} px")
        assert loops.size == 1 and pts.shape[0] == 162
        assert sub <= 0.01 and mid >= 0.4


def test_disk_polygon_area_is_the_disks():
    u = su.disk(64)
    _, pts = su.trace_subpixel(u, 8)
    area, length = su.measure(pts)
    R = su.DISKS[64][0]
    print(f"area {area:.3f} (pi R^2 = {math.pi * R * R:.3f}), length {length:.3f} (2 pi R = {2 * math.pi * R:.3f})")
    assert abs(area - math.pi * R * R) <= 0.005 * math.pi * R * R
    assert length <= 2 * math.pi * R   # (an inscribed polygon, to 0.0056 px)
    assert length >= 0.99 * 2 * math.pi * R


def test_a_reinitialised_level_set_gives_midpoints_everywhere():
    """the distance to a pixel-edge front is 0.5 on one side of every boundary edge and -0.5 on the other: t == 0.5"""
    m = ct.ring_and_blob()
    h, w = m.shape
    yy, xx = np.mgrid[0:h, 0:w]
    edges = ct.edges_of(m)
    mids = np.array([((t[0] + hd[0]) / 2 - 0.5, (t[1] + hd[1]) / 2 - 0.5) for t, hd in edges.values()])   # in pixel-centre coordinates
    d = np.sqrt(((xx[..., None] - mids[:, 0]) ** 2 + (yy[..., None] - mids[:, 1]) ** 2)).min(axis=-1)
    for (r, c) in zip(*np.nonzero(d <= 0.5)):   # (beside a boundary edge the nearest front point is that edge's midpoint, exactly 0.5 away)
        assert d[r, c] == 0.5
    u = np.where(m, d, -d)
    for conn in (4, 8):
        loops, pts, ids = su.trace_subpixel_edges(u, conn)
        k, p = ids % 4, ids // 4
        want = np.stack([(p % w) + 0.5 + su.DX[k] * 0.5, (p // w) + 0.5 + su.DY[k] * 0.5], axis=1)
        assert np.array_equal(pts, want) and np.array_equal(pts, su.midpoints(u, conn))
