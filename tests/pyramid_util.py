"""numpy restatement of the coarse-to-fine operators (include/chanvese_hip.h, "Coarse-to-fine"): restrict, prolong, the shapes of a
pyramid, the pyramid run on the CPU oracle -- and the inputs the tests share.  Both operators are defined in integers or as bit
copies, so every comparison against them is an equality.  Shared by test_pyramid_api.py (CPU) and test_gpu_pyramid.py."""
import functools
import struct

import numpy as np

# fine shapes: no tail and no clamp (16 x 16), an odd height with a one-column tail whose duplicate is dropped (17 x 33), an odd height
# with a tail of nine coarse columns (31 x 50), a plane the 2-pixel CSV kernel takes with whole 32-byte runs and a tail (64 x 144), several
# runs per row plus the clamped column alone in the tail (33 x 257)
SHAPES = [(16, 16), (17, 33), (31, 50), (64, 144), (33, 257)]
CHANNELS = [1, 3]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def coarse_shape(h, w):
    return (h + 1) // 2, (w + 1) // 2


def shapes(h, w, levels):
    """finest first; ValueError as capi.pyramid_shapes"""
    if levels < 1:
        raise ValueError("levels must be >= 1")
    out = [(h, w)]
    for _ in range(levels - 1):
        out.append(coarse_shape(*out[-1]))
    if min(out[-1]) < 16:
        raise ValueError("the coarsest side must not fall below 16")
    return out


def restrict(plane):
    """coarse(r, c) = (f(r0, c0) + f(r0, c1) + f(r1, c0) + f(r1, c1) + 2) >> 2, r1 = min(2r + 1, h - 1), c1 = min(2c + 1, w - 1)"""
    f = np.asarray(plane, dtype=np.int64)
    h, w = f.shape
    hc, wc = coarse_shape(h, w)
    r0, c0 = 2 * np.arange(hc), 2 * np.arange(wc)
    r1, c1 = np.minimum(r0 + 1, h - 1), np.minimum(c0 + 1, w - 1)
    s = f[r0][:, c0] + f[r0][:, c1] + f[r1][:, c0] + f[r1][:, c1] + 2
    return (s >> 2).astype(np.uint8)


def prolong(u, h, w):
    """fine(r, c) = coarse(r >> 1, c >> 1) on an h x w grid, as bit patterns"""
    b = bits(u)
    assert b.shape == coarse_shape(h, w)
    out = b[np.arange(h) >> 1][:, np.arange(w) >> 1]
    return np.ascontiguousarray(out).view(np.float64)


def prolong_mask(m, h, w):
    m = np.asarray(m)
    return np.ascontiguousarray(m[np.arange(h) >> 1][:, np.arange(w) >> 1])


def planes_of(kind, h, w, channels, seed=0):
    """kind: "random", "all255", "all0" """
    if kind == "all255":
        return [np.full((h, w), 255, dtype=np.uint8) for _ in range(channels)]
    if kind == "all0":
        return [np.zeros((h, w), dtype=np.uint8) for _ in range(channels)]
    rng = np.random.default_rng(1000 * h + w + 7 * channels + seed)
    return [rng.integers(0, 256, size=(h, w), dtype=np.uint8) for _ in range(channels)]


def f64(pattern):
    return struct.unpack("<d", struct.pack("<Q", pattern))[0]


# a NaN with a payload (quiet and signalling), -0.0, +-inf, a denormal, and a positive double that rounds to 0.0f (outside in the mask)
SPECIALS = np.array([0x7ff8dead0000beef, 0x7ff00000000c0de5, 0xfff8000000000001, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000,
                     0x0000000000000001, 0x800fffffffffffff, 0x3680000000000000, 0x0000000000000000], dtype=np.uint64)


def special_levelset(h, w, seed=0):
    """random doubles of both signs with every special pattern planted: in the corners, on the last row and column, and at random"""
    rng = np.random.default_rng(77 * h + w + seed)
    u = rng.standard_normal((h, w)) * 3.0
    b = u.view(np.uint64)
    spots = rng.choice(h * w, size=min(h * w, 4 * SPECIALS.size), replace=False)
    b.ravel()[spots] = np.resize(SPECIALS, spots.size)
    b[0, 0], b[0, -1], b[-1, 0], b[-1, -1] = SPECIALS[0], SPECIALS[3], SPECIALS[6], SPECIALS[8]
    b[-1, w // 2], b[h // 2, -1] = SPECIALS[1], SPECIALS[5]
    return u


def smooth_levelset(h, w):
    """an ordinary start for runs: a signed distance to a centred disk"""
    ii, jj = np.mgrid[0:h, 0:w]
    return min(h, w) / 3.0 - np.hypot(ii - h / 2.0, jj - w / 2.0)


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    union = (a | b).sum()
    return 1.0 if union == 0 else (a & b).sum() / union


def iou_either(a, b):
    """polarity-agnostic: a checkerboard start can converge to either sign"""
    return max(iou(a, b), iou(a, 1 - np.asarray(b)))


@functools.lru_cache(maxsize=None)
def oracle_proposition(n=256, noise=32, seed=3, levels=3):
    """The issue's case on the CPU oracle: synth.disk(n, noise, seed), default parameters, the checkerboard on the coarsest level.
    Returns (img, single (u, steps), [(u, steps)] per level finest first).  Computed once per process; callers must not modify it."""
    from chan_vese_amd import synth
    from oracle import cv_oracle as O
    img = synth.disk(n, noise=noise, seed=seed)
    p = O.make_params()
    u1, s1, _, _ = O.csv_run([img], O.checkerboard(n, n), p, 100000, trace=False)
    imgs = [img]
    for _ in range(levels - 1):
        imgs.append(restrict(imgs[-1]))
    out = [None] * levels
    u = O.checkerboard(*imgs[-1].shape)
    for k in range(levels - 1, -1, -1):
        if k < levels - 1:
            u = prolong(u, *imgs[k].shape)
        u, s, _, _ = O.csv_run([imgs[k]], u, p, 100000, trace=False)
        out[k] = (u, s)
    return img, (u1, s1), out
