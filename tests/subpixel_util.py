"""Restatements of the header's "Subpixel contours" (include/chanvese_hip.h) in numpy and in plain Python, and the level sets of its
tests.  trace_subpixel is the checker of tests/test_gpu_subpixel.py and of the torch and CLI tests: the loops of contour_util's tracer,
each edge recovered from two consecutive lattice points, its crossing computed in numpy FP64.  crossings_direct is a second restatement
that traces nothing (every foreground / neighbour pair, Python floats); tests/test_subpixel_restatement.py holds one against the other."""
import math

import numpy as np

import components_util as cu
import contour_util as ct

# side k of a pixel: the step to the neighbour across it, as (dx, dy) = (columns, rows)
DX = np.array([0, 1, 0, -1])
DY = np.array([-1, 0, 1, 0])
# the direction head - tail of edge k (contour_util.TAIL / HEAD) -> k, and the pixel (c, r) from the tail vertex (x, y)
SIDE_OF = {(1, 0): 0, (0, 1): 1, (-1, 0): 2, (0, -1): 3}
PIXEL_FROM_TAIL = [(0, 0), (-1, 0), (-1, -1), (0, -1)]


def as_state(u, state32=False):
    """the level set the device holds: the doubles, or with "state" = 32 the floats widened"""
    u = np.asarray(u, dtype=np.float64)
    if state32:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            u = u.astype(np.float32).astype(np.float64)
    return u


def clean_mask(u, conn, invert, min_area=0, fill_holes=0, keep_largest=False):
    f = cu.foreground(u, invert)
    if min_area or fill_holes or keep_largest:
        f = cu.clean(f, conn, min_area, fill_holes, keep_largest) != 0
    return f


def crossings(u, r, c, k, invert):
    """the header's point of edge k of pixel (r, c), for arrays of edges: float64 (n, 2) of x, y"""
    h, w = u.shape
    dx, dy = DX[k], DY[k]
    rq, cq = r + dy, c + dx
    inside = (rq >= 0) & (rq < h) & (cq >= 0) & (cq < w)
    s = -1.0 if invert else 1.0
    with np.errstate(all="ignore"):
        a = s * u[r, c]
        b = s * u[np.clip(rq, 0, h - 1), np.clip(cq, 0, w - 1)]
        d = a - b
        ok = inside & (a > 0) & (b <= 0) & np.isfinite(d)
        t = np.where(ok, a / np.where(ok, d, 1.0), 0.5)
    return np.stack([(c + 0.5) + dx * t, (r + 0.5) + dy * t], axis=1).astype(np.float64).reshape(-1, 2)


def trace_subpixel_edges(u, conn=8, invert=False, min_area=0, fill_holes=0, keep_largest=False, state32=False):
    """(loops, points, ids): trace_subpixel, and the edge id 4 (r w + c) + k of every point"""
    u = as_state(u, state32)
    f = clean_mask(u, conn, invert, min_area, fill_holes, keep_largest)
    loops, pts = ct.trace(f, conn, False)
    n = pts.shape[0]
    if not n:
        return loops, np.zeros((0, 2)), np.zeros(0, np.int64)
    nxt = np.arange(n) + 1
    ends = (loops["offset"] + loops["points"]).astype(np.int64)
    nxt[ends - 1] = loops["offset"].astype(np.int64)          # the last point of a loop is followed by its first
    step = pts[nxt].astype(np.int64) - pts
    k = np.array([SIDE_OF[(int(sx), int(sy))] for sx, sy in step])
    off = np.array(PIXEL_FROM_TAIL)[k]
    c, r = pts[:, 0] + off[:, 0], pts[:, 1] + off[:, 1]
    assert np.all(f[r, c])
    return loops, crossings(u, r, c, k, invert), 4 * (r.astype(np.int64) * u.shape[1] + c) + k


def trace_subpixel(u, conn=8, invert=False, min_area=0, fill_holes=0, keep_largest=False, state32=False):
    """(loops, points): loops as contour_util.trace(simplify=False) gives them, points float64 (P, 2) of x, y"""
    return trace_subpixel_edges(u, conn, invert, min_area, fill_holes, keep_largest, state32)[:2]


def crossings_direct(u, mask, invert):
    """{edge id: (x, y)} over ALL pairs of a foreground pixel of mask and a neighbour that is not (or lies outside): no tracing, and
    the header's rule written again, in Python floats"""
    h, w = mask.shape
    s = -1.0 if invert else 1.0
    out = {}
    for r in range(h):
        for c in range(w):
            if not mask[r, c]:
                continue
            for k, (dx, dy) in enumerate(((0, -1), (1, 0), (0, 1), (-1, 0))):
                rq, cq = r + dy, c + dx
                border = not (0 <= rq < h and 0 <= cq < w)
                if not border and mask[rq, cq]:
                    continue
                t = 0.5
                if not border:
                    a, b = s * float(u[r, c]), s * float(u[rq, cq])
                    if a > 0 and b <= 0 and math.isfinite(a - b):
                        t = a / (a - b)
                out[4 * (r * w + c) + k] = ((c + 0.5) + dx * t, (r + 0.5) + dy * t)
    return out


def check_against_direct(u, conn, invert, min_area=0, fill_holes=0, keep_largest=False, state32=False):
    """trace_subpixel against crossings_direct: the same multiset of points, the same point edge by edge, 0 <= t <= 1, and every loop's
    cyclic order by adjacency -- consecutive points belong to boundary edges that share a lattice vertex (head of one, tail of the
    next), each edge met once.  Returns (loops, points)."""
    uu = as_state(u, state32)
    f = clean_mask(uu, conn, invert, min_area, fill_holes, keep_largest)
    loops, pts, ids = trace_subpixel_edges(u, conn, invert, min_area, fill_holes, keep_largest, state32)
    direct = crossings_direct(uu, f, invert)
    assert sorted(map(tuple, pts.tolist())) == sorted(direct.values())
    assert sorted(ids.tolist()) == sorted(direct) and [direct[e] for e in ids.tolist()] == list(map(tuple, pts.tolist()))
    edges = ct.edges_of(f)
    assert int(loops["points"].sum()) == len(edges) == pts.shape[0] and np.array_equal(loops["points"], loops["edges"])
    for l in loops:
        o, n = int(l["offset"]), int(l["points"])
        cyc = ids[o:o + n].tolist()
        assert cyc[0] == int(l["first"]) == min(cyc)
        for i, e in enumerate(cyc):
            assert edges[e][1] == edges[cyc[(i + 1) % n]][0], (e, cyc[(i + 1) % n])
    w = f.shape[1]
    for e, (x, y) in direct.items():   # on the segment between the two pixel centres
        r, c = divmod(e >> 2, w)
        assert abs(x - (c + 0.5)) + abs(y - (r + 0.5)) <= 1.0 and (x == c + 0.5 or y == r + 0.5)
    return loops, pts


# ---- level sets ----
def from_mask(mask, seed=0):
    """magnitudes uniform in (0.1, 3), the sign from the mask"""
    m = np.asarray(mask).astype(bool)
    mag = np.random.default_rng(seed).uniform(0.1, 3.0, m.shape)
    return np.where(m, mag, -mag)


DISKS = {64: (20.3, 31.7, 30.2)}   # n: R and the centre (x, y), measured from the centre of pixel (0, 0)


def disk(n=64):
    """the analytic signed distance of a disk, positive inside, at the pixel centres"""
    R, cx, cy = DISKS[n]
    yy, xx = np.mgrid[0:n, 0:n]
    return R - np.sqrt((xx - cx) ** 2 + (yy - cy) ** 2)


def radial_error(points, n=64):
    """the largest | distance from the centre - R | over points in the lattice of "Contours" (pixel centres at half-integers)"""
    R, cx, cy = DISKS[n]
    p = np.asarray(points, dtype=np.float64) - 0.5
    return float(np.abs(np.sqrt((p[:, 0] - cx) ** 2 + (p[:, 1] - cy) ** 2) - R).max())


def midpoints(u, conn=8):
    """the lattice loop's edge midpoints: what a caller has without the level set (t = 0.5 everywhere)"""
    f = cu.foreground(u)
    return trace_subpixel(np.where(f, 0.5, -0.5), conn)[1]


def special(h=37, w=160, seed=3):
    """random values sprinkled with NaN, zeros of both signs, 1e-50 (positive, 0.0f as a float), infinities, and +-1e308 neighbours whose
    difference overflows.  (A float state needs a width that is a multiple of 16, at least 144.)"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((h, w)) * 3
    flat = u.reshape(-1)
    for k, v in enumerate([np.nan, -0.0, 0.0, 1e-50, -1e-50, np.inf, -np.inf, 1e308, -1e308]):
        flat[(k * 7919 + 1) % flat.size::max(flat.size // 13, 1) + k] = v
    u[5, 20:28] = [1e308, -1e308, 1e308, -1e308, np.inf, -1e308, 1e308, -np.inf]   # a - b overflows; an infinite a; an infinite b
    u[6, 20:28] = [-1e308, 1e308, -0.0, 1.0, 0.0, 1.0, 1e-50, 1.0]
    u[7, 20:24] = [np.nan, 1.0, -1.0, np.nan]
    return u


def measure(points):
    """cvh_contour_subpixel_measure in Python floats: (area, length) of one loop's points, summed left to right in index order"""
    p = [(float(x), float(y)) for x, y in np.asarray(points, dtype=np.float64).reshape(-1, 2).tolist()]
    cross, length = 0.0, 0.0
    for i, (x0, y0) in enumerate(p):
        x1, y1 = p[(i + 1) % len(p)]
        cross += x0 * y1 - x1 * y0
        dx, dy = x1 - x0, y1 - y0
        length += math.sqrt(dx * dx + dy * dy)
    return 0.5 * cross, length
