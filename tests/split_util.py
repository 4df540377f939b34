"""Two independent restatements of "Object split" (include/chanvese_hip.h), the cut, the table and the cases the split tests share.

1. split_numpy: scipy's binary_erosion(border_value=1) by the disk and scipy's label for F0's components and for the markers, then
   SYNCHRONOUS rounds of the lexicographic minimum over (d, L) keys held as one int64 each.
2. split_queue: plain Python and nothing else -- its own erosion by offsets, its own flood-fill labelling in raster order, a breadth-first
   queue from the markers for d, then the labels in order of d.
Nothing here touches the library."""
import functools
from collections import deque

import numpy as np

import components_util as CU
import morph_util as M

INF = np.int64(0x3FFFFFFF) << 32   # (INF + ONE stays an int64)
ONE = np.int64(1) << 32


def _shifts(conn):
    return [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])


def _structure(conn):
    return np.ones((3, 3), bool) if conn == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)


def shifted(a, dy, dx, fill):
    """b[p] = a[p + (dy, dx)], `fill` where that lies outside the plane"""
    h, w = a.shape
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, max(h - dy, 0))) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, max(w - dx, 0))) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    b[yd, xd] = a[ys, xs]
    return b


def reach(r2, h, w):
    """no two pixels of the plane are farther apart than its diagonal: a larger disk is the same operator"""
    return min(int(r2), (h - 1) ** 2 + (w - 1) ** 2)


def markers_numpy(f0, conn, r2):
    """(E, M): the eroded set and the marker set"""
    from scipy import ndimage
    f0 = np.asarray(f0, bool)
    r2 = reach(r2, *f0.shape)
    e = ndimage.binary_erosion(f0, M.disk_structure(r2), border_value=1) if r2 > 0 else f0.copy()
    lab, k = ndimage.label(f0, _structure(conn))
    has = np.zeros(k + 1, bool)
    has[np.unique(lab[e])] = True
    has[0] = True
    return e, e | (f0 & ~has[lab])


def relax_round(key, f0, conn):
    """one synchronous round: key(p) = min(key(p), min_q key(q) + ONE) over the conn-neighbours q in F0; keys outside F0 stay 0"""
    best = key.copy()
    src = np.where(f0, key, INF)   # (a neighbour outside F0 offers nothing; INF + ONE stays above INF)
    for dy, dx in _shifts(conn):
        best = np.minimum(best, shifted(src, dy, dx, INF) + ONE)
    return np.where(f0, best, 0)


def start_keys(f0, m, conn):
    from scipy import ndimage
    lab, k = ndimage.label(m, _structure(conn))   # raster order of first pixels: cvh_components' numbering
    return np.where(m, lab.astype(np.int64), np.where(f0, INF, np.int64(0))), k


def split_numpy(f0, conn, r2):
    """(L int32, K, rounds)"""
    f0 = np.asarray(f0, bool)
    _, m = markers_numpy(f0, conn, r2)
    key, k = start_keys(f0, m, conn)
    rounds = 0
    while True:
        nxt = relax_round(key, f0, conn)
        if np.array_equal(nxt, key):
            break
        key, rounds = nxt, rounds + 1
    assert not (key == INF).any()   # every pixel of F0 is reached
    return (key & 0xFFFFFFFF).astype(np.int32), k, rounds


def relax_random(f0, conn, r2, seed):
    """the keys after relaxing single pixels in a random order until a full pass changes nothing: (keys, keys of the synchronous rounds)"""
    f0 = np.asarray(f0, bool)
    _, m = markers_numpy(f0, conn, r2)
    key, _ = start_keys(f0, m, conn)
    sync = key.copy()
    while True:
        nxt = relax_round(sync, f0, conn)
        if np.array_equal(nxt, sync):
            break
        sync = nxt
    h, w = f0.shape
    rng = np.random.default_rng(seed)
    todo = [(i, j) for i in range(h) for j in range(w) if f0[i, j] and not m[i, j]]
    key = key.copy()
    changed = True
    while changed:
        changed = False
        for t in rng.permutation(len(todo)):
            i, j = todo[t]
            best = key[i, j]
            for dy, dx in _shifts(conn):
                y, x = i + dy, j + dx
                if 0 <= y < h and 0 <= x < w and f0[y, x]:
                    best = min(best, key[y, x] + ONE)
            if best < key[i, j]:
                key[i, j], changed = best, True
    return key, sync


# ---- the sequential restatement: no numpy operation beyond indexing, no scipy ----
def _flood_label(m, conn):
    h, w = len(m), len(m[0])
    lab = [[0] * w for _ in range(h)]
    k = 0
    for i in range(h):
        for j in range(w):
            if not m[i][j] or lab[i][j]:
                continue
            k += 1
            lab[i][j] = k
            q = deque([(i, j)])
            while q:
                y, x = q.popleft()
                for dy, dx in _shifts(conn):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and m[yy][xx] and not lab[yy][xx]:
                        lab[yy][xx] = k
                        q.append((yy, xx))
    return lab, k


def split_queue(f0, conn, r2):
    """(L int32, K)"""
    f = np.asarray(f0, bool).tolist()
    h, w = len(f), len(f[0])
    offs = M.disk_offsets(reach(r2, h, w))
    e = [[f[i][j] and all(f[i + dy][j + dx] for dy, dx in offs if 0 <= i + dy < h and 0 <= j + dx < w) for j in range(w)] for i in range(h)]
    comp, kc = _flood_label(f, conn)
    has = [False] * (kc + 1)
    for i in range(h):
        for j in range(w):
            if e[i][j]:
                has[comp[i][j]] = True
    m = [[f[i][j] and (e[i][j] or not has[comp[i][j]]) for j in range(w)] for i in range(h)]
    lab, k = _flood_label(m, conn)
    d = [[0 if m[i][j] else -1 for j in range(w)] for i in range(h)]
    q = deque((i, j) for i in range(h) for j in range(w) if m[i][j])
    order = []
    while q:
        y, x = q.popleft()
        for dy, dx in _shifts(conn):
            yy, xx = y + dy, x + dx
            if 0 <= yy < h and 0 <= xx < w and f[yy][xx] and d[yy][xx] < 0:
                d[yy][xx] = d[y][x] + 1
                q.append((yy, xx))
                order.append((yy, xx))
    for y, x in order:   # breadth-first order is the order of d: every pixel at d - 1 has its label already
        lab[y][x] = min(lab[y + dy][x + dx] for dy, dx in _shifts(conn)
                        if 0 <= y + dy < h and 0 <= x + dx < w and f[y + dy][x + dx] and d[y + dy][x + dx] == d[y][x] - 1)
    assert all(d[i][j] >= 0 for i in range(h) for j in range(w) if f[i][j])
    return np.array(lab, np.int32).reshape(h, w), k


def cut_of(lab):
    """cut(p) <=> L(p) > 0 and some 8-neighbour has a larger label"""
    lab = np.asarray(lab, np.int64)
    top = np.zeros_like(lab)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                top = np.maximum(top, shifted(lab, dy, dx, 0))
    return (lab > 0) & (top > lab)


def table_of(lab, m, conn, k):
    """row k - 1: first the smallest flat index of marker k, area and inclusive box of { L = k }"""
    from scipy import ndimage
    mlab, km = ndimage.label(m, _structure(conn))
    assert km == k
    tab = np.zeros(k, CU.COMPONENT_DTYPE)
    flat = mlab.ravel()
    for n in range(1, k + 1):
        ys, xs = np.nonzero(lab == n)
        tab[n - 1] = (int(np.flatnonzero(flat == n)[0]), ys.size, xs.min(), ys.min(), xs.max(), ys.max())
    return tab


class Split:
    """everything a test compares against, for one (F0, conn, r2)"""
    def __init__(self, f0, conn, r2):
        self.f0 = np.asarray(f0, bool)
        self.eroded, self.markers = markers_numpy(self.f0, conn, r2)
        self.labels, self.K, self.rounds = split_numpy(self.f0, conn, r2)
        self.cut = cut_of(self.labels)
        self.table = table_of(self.labels, self.markers, conn, self.K)
        self.pieces = self.f0 & ~self.cut
        for a in (self.f0, self.labels, self.cut, self.table, self.pieces):
            a.setflags(write=False)


def start_set(u, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False):
    """F0 of a level set: cvh_get_mask_clean's set"""
    return CU.clean(M.mask_of(u, invert), conn, min_area, fill_holes, keep_largest).astype(bool)


@functools.lru_cache(maxsize=None)
def expected(name, h, w, conn, r2, invert=False, clean=(0, 0, False)):
    return Split(start_set(case(name, h, w), conn, invert, *clean), conn, r2)


# ---- the cases ----
def demonstration():
    """64 x 64: two overlapping disks of radius 12, a 3 x 3 square and a two-row bar"""
    y, x = np.mgrid[0:64, 0:64]
    m = ((x - 23) ** 2 + (y - 30) ** 2 <= 144) | ((x - 41) ** 2 + (y - 34) ** 2 <= 144)
    m[5:8, 5:8] = True
    m[50:52, 10:40] = True
    return m


def spiral(h, w):
    """a 3 x 3 block at the plane's centre and a one-pixel-wide corridor that winds outwards from it, one pixel of wall between its
    turns, until it meets the plane's border: (mask, the block's centre).  Eroded by the cross (r2 = 1) the block's centre and its
    neighbour towards the corridor are the only marker, and the growth has the whole corridor to travel."""
    cy, cx = h // 2, w // 2
    m = np.zeros((h, w), bool)
    m[cy - 1:cy + 2, cx - 1:cx + 2] = True
    pos = [cy, cx + 1]

    def go(ty, tx):
        while (pos[0], pos[1]) != (ty, tx):
            y, x = pos[0] + np.sign(ty - pos[0]), pos[1] + np.sign(tx - pos[1])
            if not (0 <= y < h and 0 <= x < w):
                return False
            pos[0], pos[1] = int(y), int(x)
            m[y, x] = True
        return True

    ok, k = go(cy, cx + 3), 3
    while ok:
        ok = go(cy + k, cx + k) and go(cy + k, cx - k) and go(cy - k, cx - k) and go(cy - k, cx + k + 2)
        k += 2
    return m, (cy, cx)


def _touching(h, w):
    """a field of overlapping disks, as far as the plane holds them, and speckle"""
    rng = np.random.default_rng(h * 131 + w)
    m = np.zeros((h, w), bool)
    r = max(2, min(h, w) // 8)
    for cy in range(r, h, 2 * r - 1):
        for cx in range(r, w, 2 * r - 2):
            m |= M.disk(h, w, cy + int(rng.integers(-1, 2)), cx, r)
    return m ^ (rng.random((h, w)) < 0.01)


def _demo(h, w):
    m = np.zeros((h, w), bool)
    d = demonstration()
    m[:min(h, 64), :min(w, 64)] = d[:min(h, 64), :min(w, 64)]
    return m


CASES = {
    "touching": _touching,
    "demo": _demo,
    "noisy": lambda h, w: np.random.default_rng(7 * h + w).random((h, w)) < 0.6,
    "all_inside": lambda h, w: np.ones((h, w), bool),
    "all_outside": lambda h, w: np.zeros((h, w), bool),
}
R2S = (0, 1, 4, 9, 2 ** 32 - 1)
SMALL_SHAPES = [(1, 7), (7, 1), (2, 2), (9, 21)]


def shapes(tile_rows, tile_cols):
    """one tile, one row past a tile, one column past a tile, two tiles each way, a width that is no multiple of the 16-byte piece"""
    return [(tile_rows, tile_cols), (tile_rows + 1, tile_cols), (tile_rows, tile_cols + 1), (2 * tile_rows, 2 * tile_cols), (tile_rows + 5, tile_cols + 7)]


@functools.lru_cache(maxsize=None)
def case(name, h, w):
    """the case's level set (its mask is the case's set): computed once, shared, read-only"""
    u = np.ascontiguousarray(M.levelset_of(CASES[name](h, w), np.random.default_rng(11)), dtype=np.float64)
    u.setflags(write=False)
    return u
