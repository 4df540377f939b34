"""The restatement of "Mask morphology" (include/chanvese_hip.h) in exact integers, and the shapes, cases and squared radii the
morphology tests share.

dilate by shifted ORs over D(r2) = {dx^2 + dy^2 <= r2} with the header's border rule (what lies outside the plane belongs to neither
set), erode as its dual under complement within the plane; for radii whose disk has too many offsets to shift, an exact integer two-pass
minimum -- columns (nearest set row of every column), then rows (min over k of k^2 + g^2) -- thresholded at r2.  Nothing here touches the
library, and nothing here needs scipy."""
import functools
import math

import numpy as np

NONE, DILATE, ERODE, OPEN, CLOSE = range(5)
OPS = (NONE, DILATE, ERODE, OPEN, CLOSE)
OP_NAMES = {NONE: "none", DILATE: "dilate", ERODE: "erode", OPEN: "open", CLOSE: "close"}
# 1 x 1, a single row, 16 x 16 (lane tail), 33 x 257 (one row past a band, one column past a chunk of 256), 65 x 31 (three bands,
# narrow), 64 x 144, 96 x 300
SHAPES = [(1, 1), (1, 70), (16, 16), (33, 257), (65, 31), (64, 144), (96, 300)]
CHANNELS = (1, 3)
R2S = (0, 1, 2, 4, 5, 8, 9, 25, 100, 2 ** 32 - 1)
SHIFT_LIMIT = 100          # squared radii up to here are restated by shifts (317 offsets at 100), larger ones by the two-pass minimum



def mask_of(u, invert=False):
    """cvh_get_mask's rule: ((float)u > 0) != invert"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (np.asarray(u, dtype=np.float64).astype(np.float32) > 0) != bool(invert)


def levelset_of(m, rng=None):
    """a level set whose mask is m: +-(0.25 .. 4), magnitudes seeded"""
    mag = np.ones(m.shape) if rng is None else rng.uniform(0.25, 4.0, size=m.shape)
    return np.where(m, mag, -mag)


def planes_of(h, w, channels, seed=3):
    return [p for p in np.random.default_rng(seed).integers(0, 256, size=(channels, h, w), dtype=np.uint8)]


def disk(h, w, cy, cx, r):
    y, x = np.mgrid[0:h, 0:w]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def isqrt(r2):
    return math.isqrt(int(r2))


def disk_offsets(r2):
    r = isqrt(r2)
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= r2]


def disk_structure(r2):
    """D(r2) as the boolean (2 r + 1)^2 structuring element scipy takes"""
    r = isqrt(r2)
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return y * y + x * x <= r2


def dilate_shifts(f, r2):
    f = np.asarray(f, dtype=bool)
    h, w = f.shape
    out = np.zeros_like(f)
    for dy, dx in disk_offsets(r2):
        if abs(dy) >= h or abs(dx) >= w:
            continue
        # out[p] |= f[p + d] where p + d lies in the plane
        ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
        xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
        out[yd, xd] |= f[ys, xs]
    return out


def squared_distance(f):
    """exact squared Euclidean distance of every pixel to the nearest pixel of f, int64; -1 where f is empty.  Two passes of integer
    minima: the nearest set row of every column, then min over the row's columns of (column distance)^2 + g^2"""
    f = np.asarray(f, dtype=bool)
    h, w = f.shape
    big = np.int64(1) << 40
    rows = np.arange(h, dtype=np.int64)[:, None]
    up = np.maximum.accumulate(np.where(f, rows, -big), axis=0)                           # nearest set row at or above
    down = np.minimum.accumulate(np.where(f, rows, big)[::-1], axis=0)[::-1]              # at or below
    g = np.minimum(rows - up, down - rows)
    g2 = np.where(g >= big // 2, big, g * g)
    cols = np.arange(w, dtype=np.int64)
    k2 = (cols[:, None] - cols[None, :]) ** 2                                             # [j, j']
    d2 = np.empty((h, w), dtype=np.int64)
    for i in range(h):
        d2[i] = (k2 + g2[i][None, :]).min(axis=1)
    return np.where(d2 >= big, -1, d2)


def dilate(f, r2):
    f = np.asarray(f, dtype=bool)
    if r2 <= SHIFT_LIMIT:
        return dilate_shifts(f, r2)
    d2 = squared_distance(f)
    return (d2 >= 0) & (d2 <= r2)


def erode(f, r2):
    """P \\ dilate(P \\ F): only background pixels OF THE PLANE erode"""
    return ~dilate(~np.asarray(f, dtype=bool), r2)


def morph(f, op, r2):
    """the header's op on the boolean plane f"""
    f = np.asarray(f, dtype=bool)
    if op == NONE or r2 == 0:
        return f.copy()
    if op == DILATE:
        return dilate(f, r2)
    if op == ERODE:
        return erode(f, r2)
    if op == OPEN:
        return dilate(erode(f, r2), r2)
    if op == CLOSE:
        return erode(dilate(f, r2), r2)
    raise ValueError(op)


# ---- the cases: name -> level set for a shape (the set is mask_of(u)) ----
def _noisy(h, w):
    return np.random.default_rng(1000 * h + w).normal(size=(h, w))


def _disks(h, w):
    r = max(2, min(h, w) // 3)
    m = disk(h, w, h // 2, w // 2, r) | disk(h, w, 2, w - 3, 3)
    m &= ~disk(h, w, h // 2, w // 2, max(1, r // 3))                  # a hole
    return levelset_of(m, np.random.default_rng(5))


def _checker(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return levelset_of((y + x) % 2 == 0)


def _corners(h, w):
    m = np.zeros((h, w), bool)
    m[0, 0] = m[h - 1, w - 1] = True
    return levelset_of(m)


def bridge_geometry(h, w):
    """two blocks joined by a one-pixel-wide bridge along row `row`, columns c0 .. c1 - 1 (None where the plane is too small)"""
    if h < 9 or w < 15:
        return None
    row, c0, c1 = h // 2, w // 2 - 2, w // 2 + 2
    return row, c0, c1


def _bridge(h, w):
    m = np.zeros((h, w), bool)
    geo = bridge_geometry(h, w)
    if geo is None:
        m[h // 2, :] = True                                             # a one-pixel line: all bridge
        return levelset_of(m)
    row, c0, c1 = geo
    m[row - 3:row + 4, 1:c0] = True
    m[row - 3:row + 4, c1:w - 1] = True
    m[row, c0:c1] = True
    return levelset_of(m)


def crack_geometry(h, w):
    """a block split by a one-pixel-wide crack down column `col`, rows r0 .. r1 - 1 (None where the plane is too small)"""
    if h < 9 or w < 9:
        return None
    return w // 2, 1, h - 1


def _crack(h, w):
    m = np.ones((h, w), bool)
    geo = crack_geometry(h, w)
    if geo is None:
        m[:, w // 2] = False
        return levelset_of(m)
    col, r0, r1 = geo
    m[r0:r1, col] = False
    return levelset_of(m)


def _band_seam(h, w):
    """rows 0 .. 31 set (or the upper half of a lower plane): row 31 dilates into row 32 and row 32's background erodes row 31"""
    m = np.zeros((h, w), bool)
    m[:(31 if h > 32 else max(h // 2 - 1, 0)) + 1, :] = True
    if h > 40:
        m[40, w // 2] = True                                            # and a single pixel whose disk crosses the seam upwards
    return levelset_of(m)


def _column_seam(h, w):
    """the same across columns 255 / 256 (or the middle of a narrower plane)"""
    m = np.zeros((h, w), bool)
    c = 255 if w > 256 else max(w // 2 - 1, 0)
    m[:, :c + 1] = True
    return levelset_of(m)


def _mask_rule(h, w):
    """NaN, -0.0, +-inf and a positive double that rounds to 0.0f, scattered over a noisy level set"""
    rng = np.random.default_rng(77)
    u = rng.normal(size=(h, w))
    flat = u.reshape(-1)
    specials = [np.nan, -0.0, 0.0, np.inf, -np.inf, 1e-60, -1e-60]
    k = min(flat.size // 2, 90)
    flat[rng.choice(flat.size, size=k, replace=False)] = np.resize(specials, k)
    return u


CASES = {
    "noisy": _noisy, "disks": _disks, "checker": _checker, "corners": _corners, "bridge": _bridge, "crack": _crack, "band_seam": _band_seam,
    "column_seam": _column_seam, "all_inside": lambda h, w: np.full((h, w), 1.5), "all_outside": lambda h, w: np.full((h, w), -1.5),
    "mask_rule": _mask_rule,
}


@functools.lru_cache(maxsize=None)
def case(name, h, w):
    """the case's level set: computed once, shared, read-only"""
    u = np.ascontiguousarray(CASES[name](h, w), dtype=np.float64)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def expected(name, h, w, invert, op, r2):
    """the restated 0/1 bytes of a case: computed once, shared, read-only"""
    out = morph(mask_of(case(name, h, w), invert), op, r2).astype(np.uint8)
    out.setflags(write=False)
    return out


def noisy_disk(h, w, seed=3):
    """a disk with speckle inside and out: what opening and closing are for"""
    rng = np.random.default_rng(seed)
    m = disk(h, w, h // 2, w // 2, min(h, w) // 3)
    return m ^ (rng.random((h, w)) < 0.03)
