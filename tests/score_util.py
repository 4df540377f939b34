"""The restatement of "Mask scores" (include/chanvese_hip.h) in numpy / scipy, the shapes and the cases the score tests share.

Surface by the header's scipy formula; d2 by brute force in int64 over all pairs surface x surface (the test shapes are small enough);
q16 as np.rint(np.sqrt(d2.astype(np.float64)) * 65536).astype(np.uint64).  Nothing here touches the library."""
import functools

import numpy as np
from scipy import ndimage

FIELDS = ("tp", "fp", "fn", "tn", "surf_m", "surf_t", "within_m", "within_t", "dist_m_q16", "dist_t_q16", "hd2_m", "hd2_t", "defined")
CROSS = ndimage.generate_binary_structure(2, 1)
# 16 x 16 (lane tail), 33 x 257 (one row past a band, one column past a chunk of 256), 65 x 31 (three bands, narrow), 64 x 144, 96 x 300
SHAPES = [(16, 16), (33, 257), (65, 31), (64, 144), (96, 300)]
CHANNELS = (1, 3)
TOL2S = (0, 4, "beyond")          # "beyond": a value above h^2 + w^2


def mask_of(u, invert=False):
    """cvh_get_mask's rule: ((float)u > 0) != invert"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(u, dtype=np.float64).astype(np.float32) > 0) != bool(invert)


def surface(s):
    s = np.asarray(s, dtype=bool)
    return s & ~ndimage.binary_erosion(s, CROSS, border_value=0)


def directed_d2(a, b):
    """for every pixel of a (row-major order), the smallest squared distance to a pixel of b: int64, all pairs"""
    pa, pb = np.argwhere(a).astype(np.int64), np.argwhere(b).astype(np.int64)
    out = np.empty(len(pa), dtype=np.int64)
    yb, xb = pb[None, :, 0], pb[None, :, 1]
    step = max(1, (1 << 18) // max(len(pb), 1))          # blocks that stay in cache
    for k in range(0, len(pa), step):
        dy, dx = pa[k:k + step, 0, None] - yb, pa[k:k + step, 1, None] - xb
        dy *= dy
        dx *= dx
        dy += dx
        out[k:k + step] = dy.min(axis=1)
    return out


def q16(d2):
    return np.rint(np.sqrt(d2.astype(np.float64)) * 65536).astype(np.uint64)


def tol2_value(tol2, h, w):
    return h * h + w * w + 7 if tol2 == "beyond" else int(tol2)


def distances(m, t):
    """(d2 over surf(M) against surf(T), d2 over surf(T) against surf(M)), or None where a surface is empty"""
    sm, st = surface(m), surface(t)
    if not sm.any() or not st.any():
        return None
    return directed_d2(sm, st), directed_d2(st, sm)


def score(m, t, tol2, dist=None):
    """the thirteen integers of cvh_mask_score for the boolean planes m (mask) and t (truth), as a dict of Python ints"""
    m, t = np.asarray(m, dtype=bool), np.asarray(t, dtype=bool)
    sm, st = surface(m), surface(t)
    out = dict(tp=int((m & t).sum()), fp=int((m & ~t).sum()), fn=int((~m & t).sum()), tn=int((~m & ~t).sum()),
               surf_m=int(sm.sum()), surf_t=int(st.sum()))
    out.update(within_m=0, within_t=0, dist_m_q16=0, dist_t_q16=0, hd2_m=0, hd2_t=0, defined=int(sm.any() and st.any()))
    if out["defined"]:
        dm, dt = dist if dist is not None else distances(m, t)
        out.update(within_m=int((dm <= tol2).sum()), within_t=int((dt <= tol2).sum()), dist_m_q16=int(q16(dm).sum(dtype=np.uint64)),
                   dist_t_q16=int(q16(dt).sum(dtype=np.uint64)), hd2_m=int(dm.max()), hd2_t=int(dt.max()))
    return out


def as_dict(s):
    """a capi.Score or capi.MaskScore as the restatement's dict"""
    return {f: int(getattr(s, f)) for f in FIELDS}


def disk(h, w, cy, cx, r):
    y, x = np.mgrid[0:h, 0:w]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def levelset_of(m, rng=None):
    """a level set whose mask is m: +-(0.25 .. 4), magnitudes seeded"""
    mag = np.ones(m.shape) if rng is None else rng.uniform(0.25, 4.0, size=m.shape)
    return np.where(m, mag, -mag)


# ---- the cases: name -> (level set, truth bytes) for a shape ----
def _noisy(h, w):
    rng = np.random.default_rng(1000 * h + w)
    return rng.normal(size=(h, w)), (rng.random((h, w)) < 0.4).astype(np.uint8) * rng.integers(1, 256, size=(h, w), dtype=np.uint8)


def _disks(h, w):
    r = max(2, min(h, w) // 3)
    return levelset_of(disk(h, w, h // 2, w // 2, r), np.random.default_rng(5)), disk(h, w, h // 2 + 1, w // 2 + 3, r).astype(np.uint8) * 255


def _checker(h, w):
    y, x = np.mgrid[0:h, 0:w]
    c = (y + x) % 2 == 0
    return levelset_of(c), (~c).astype(np.uint8)


def _identical(h, w):
    m = disk(h, w, h // 2, w // 3, max(2, min(h, w) // 4)) | disk(h, w, 2, w - 3, 4)
    return levelset_of(m), m.astype(np.uint8) * 7


def _corners(h, w):
    m, t = np.zeros((h, w), bool), np.zeros((h, w), np.uint8)
    m[0, 0], t[h - 1, w - 1] = True, 1
    return levelset_of(m), t


def _band_seam(h, w):
    """a surface pixel in row 31 whose only neighbour of the other kind is in row 32 (M: rows 0 .. 31 of a column strip, its lower edge
    faces row 32), and the truth the same across the band seam the other way; needs h > 33"""
    m, t = np.zeros((h, w), bool), np.zeros((h, w), np.uint8)
    r = min(31, h - 2)
    m[:r + 1, :] = True                       # full rows 0 .. r: row r is surface only because row r + 1 is outside
    t[r + 1:, :] = 1                          # rows r + 1 .. h - 1: row r + 1 is surface only because row r is outside
    return levelset_of(m), t


def _column_seam(h, w):
    """the same across columns 255 / 256 (or the middle of a narrower plane)"""
    m, t = np.zeros((h, w), bool), np.zeros((h, w), np.uint8)
    c = 255 if w > 256 else w // 2 - 1
    m[:, :c + 1] = True
    t[:, c + 1:] = 1
    return levelset_of(m), t


def _mask_rule(h, w):
    """NaN, -0.0, +-inf and a positive double that rounds to 0.0f, scattered over a noisy level set"""
    rng = np.random.default_rng(77)
    u = rng.normal(size=(h, w))
    flat = u.reshape(-1)
    specials = [np.nan, -0.0, 0.0, np.inf, -np.inf, 1e-60, -1e-60]
    flat[rng.choice(flat.size, size=min(flat.size // 2, 90), replace=False)] = np.resize(specials, min(flat.size // 2, 90))
    return u, (rng.random((h, w)) < 0.5).astype(np.uint8)


def _const(u_value, t_value):
    return lambda h, w: (np.full((h, w), u_value), np.full((h, w), t_value, np.uint8))


def _truth_only(t_value):
    return lambda h, w: (_disks(h, w)[0], np.full((h, w), t_value, np.uint8))


def _u_only(u_value):
    return lambda h, w: (np.full((h, w), u_value), _disks(h, w)[1])


CASES = {
    "noisy": _noisy, "disks": _disks, "checker": _checker, "identical": _identical, "truth_zero": _truth_only(0), "truth_255": _truth_only(255),
    "all_inside": _u_only(1.5), "all_outside": _u_only(-1.5), "both_empty": _const(-1.0, 0), "corners": _corners, "band_seam": _band_seam,
    "column_seam": _column_seam, "mask_rule": _mask_rule,
}


@functools.lru_cache(maxsize=None)
def case(name, h, w):
    """(level set, truth bytes): computed once, shared, read-only"""
    u, t = CASES[name](h, w)
    u, t = np.ascontiguousarray(u, dtype=np.float64), np.ascontiguousarray(t, dtype=np.uint8)
    u.setflags(write=False)
    t.setflags(write=False)
    return u, t


@functools.lru_cache(maxsize=None)
def expected(name, h, w, invert, tol2):
    """the restatement's dict for a case; the all-pairs distances are taken once per (case, shape, invert)"""
    u, t = case(name, h, w)
    return score(mask_of(u, invert), t != 0, tol2_value(tol2, h, w), _distances(name, h, w, invert))


@functools.lru_cache(maxsize=None)
def _distances(name, h, w, invert):
    u, t = case(name, h, w)
    return distances(mask_of(u, invert), t != 0)


def planes_of(h, w, channels, seed=3):
    return [p for p in np.random.default_rng(seed).integers(0, 256, size=(channels, h, w), dtype=np.uint8)]
