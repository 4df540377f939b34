"""Sequential restatement of the header's "Contours" (include/chanvese_hip.h) in plain Python: the boundary edges of a mask, the successor
rule followed edge by edge, the loops sorted by their smallest edge.  It is the checker of tests/test_gpu_contour.py and of the torch and
CLI tests; tests/test_contour_restatement.py holds it against properties that do not use its code.  It also holds the case list."""
import numpy as np

import components_util as cu
from chan_vese_amd.capi import CONTOUR_LOOP_DTYPE as LOOP_DTYPE   # struct cvh_contour_loop (tests/test_contour_api.py pins its layout)

# edge k of pixel (r, c): the neighbour across it (dr, dc), its tail and head vertices as offsets (dx, dy) from (c, r)
ACROSS = [(-1, 0), (0, 1), (1, 0), (0, -1)]
TAIL = [(0, 0), (1, 0), (1, 1), (0, 1)]
HEAD = [(1, 0), (1, 1), (0, 1), (0, 0)]


def edges_of(mask):
    """{edge id: (tail, head)} of the boundary edges, ids ascending."""
    m = np.asarray(mask).astype(bool)
    h, w = m.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = m
    out = {}
    for r, c in zip(*np.nonzero(m)):
        r, c = int(r), int(c)
        for k in range(4):
            if not pad[r + 1 + ACROSS[k][0], c + 1 + ACROSS[k][1]]:
                out[4 * (r * w + c) + k] = ((c + TAIL[k][0], r + TAIL[k][1]), (c + HEAD[k][0], r + HEAD[k][1]))
    return out


def trace(mask, conn=8, simplify=True):
    """(loops, points): loops a structured array (LOOP_DTYPE), points int32 (P, 2) of x, y."""
    assert conn in (4, 8)
    edges = edges_of(mask)
    leaving = {}
    for e, (tail, _) in edges.items():
        leaving.setdefault(tail, []).append(e)
    succ = {}
    for e, (_, head) in edges.items():
        cands = leaving[head]
        if len(cands) == 1:
            succ[e] = cands[0]
        else:   # two foreground pixels meet diagonally: the left turn for conn 8, the right turn for conn 4
            assert len(cands) == 2
            turn = (e % 4 + (3 if conn == 8 else 1)) % 4
            (succ[e],) = [x for x in cands if x % 4 == turn]
    assert sorted(succ.values()) == sorted(edges)   # one predecessor each
    seen, rows, pts = set(), [], []
    for first in sorted(edges):
        if first in seen:
            continue
        cycle, e = [], first
        while e not in seen:
            seen.add(e)
            cycle.append(e)
            e = succ[e]
        assert e == first
        area2 = sum(edges[x][0][0] * edges[x][1][1] - edges[x][1][0] * edges[x][0][1] for x in cycle)
        keep = [x for i, x in enumerate(cycle) if not simplify or cycle[i - 1] % 4 != x % 4]
        rows.append((first, len(cycle), len(keep), 0, len(pts), area2))
        pts.extend(edges[x][0] for x in keep)
    return np.array(rows, dtype=LOOP_DTYPE), np.array(pts, dtype=np.int32).reshape(-1, 2)


def trace_clean(mask, conn=8, simplify=True, min_area=0, fill_holes=0, keep_largest=False):
    if min_area or fill_holes or keep_largest:
        mask = cu.clean(mask, conn, min_area, fill_holes, keep_largest) != 0
    return trace(mask, conn, simplify)


def assert_equal(got, want, what=""):
    """every field of every loop row and every point, =="""
    (gl, gp), (wl, wp) = got, want
    assert gl.size == wl.size, (what, gl.size, wl.size)
    for f in LOOP_DTYPE.names:
        assert np.array_equal(gl[f], wl[f]), (what, f, gl[f][:8], wl[f][:8])
    assert gp.shape == wp.shape and gp.dtype == np.int32 and np.array_equal(gp, wp), (what, gp[:8], wp[:8])


# ---- the masks of the issue's cases ----
def ring_and_blob():
    m = np.zeros((24, 40), bool)
    m[4:15, 6:20] = True
    m[8:11, 10:16] = False     # a hole that touches nothing
    m[16:24, 30:40] = True     # a blob in the corner of the plane
    m[0, 20:25] = True
    return m


def noise(h=192, w=320, seed=11):
    return np.random.default_rng(seed).random((h, w)) < 0.5


def small_masks():
    """name -> mask: everything but the noise plane"""
    gaps = np.array([[1, 0, 1, 1, 0, 0, 1]], bool)
    board = (np.add.outer(np.arange(9), np.arange(9)) % 2) == 0
    return {
        "1x1": np.ones((1, 1), bool),
        "1x7_gaps": gaps,
        "7x1_gaps": gaps.T.copy(),
        "2x2_diagonal": np.array([[1, 0], [0, 1]], bool),
        "2x2_antidiagonal": np.array([[0, 1], [1, 0]], bool),
        "9x9_checkerboard": board,
        "full": np.ones((13, 21), bool),
        "empty": np.zeros((13, 21), bool),
        "ring_and_blob": ring_and_blob(),
        "comb64": cu.comb(64, 64),
    }
