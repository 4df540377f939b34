"""Restatements of the smoothing calls (include/chanvese_hip.h, "Smoothing"), the Gaussian's taps in numpy, the kernels and the cases
the tests share.  Two independent restatements of the header's integer definition: np.pad(mode='edge') with int64 sums of shifted
slices, and scipy.ndimage.correlate1d on int64 with mode='nearest'.  The definition is in integers, so every comparison against it is
an equality.  Shared by test_smooth_restatement.py, test_smooth_api.py, test_cli_smooth.py (CPU), test_gpu_smooth.py and
test_gpu_torch_smooth.py."""
import functools
import math

import numpy as np

from local_util import blocky_planes, random_planes

COPY, BLUR, DETAIL = 0, 1, 2
NAMES = {"blur": BLUR, "detail": DETAIL}
RADIUS_MAX, TAP_SUM = 63, 32768
# smooth_kernels.hip: a workgroup of the column pass takes band_rows(R) rows x STRIP columns per trip (its LDS tile holds TILE_ROWS rows:
# the band and R rows on either side), a workgroup of the row pass SEGMENT columns of a row (test_smooth_api.py compares these numbers
# with the library's cvh_debug_smooth_geometry)
TILE_ROWS, STRIP, SEGMENT = 256, 64, 1024


def band_rows(R):
    return TILE_ROWS - 2 * R


def full_taps(taps):
    """t[-R .. R] as int64"""
    t = np.asarray(taps, dtype=np.int64)
    return np.concatenate([t[:0:-1], t])


def row_sums(plane, taps):
    """a(x, y): the tap-weighted sums along a row, border replicated, before the rounding"""
    R = len(taps) - 1
    p = np.pad(np.asarray(plane).astype(np.int64), ((0, 0), (R, R)), mode="edge")
    w = plane.shape[1]
    return sum(int(t) * p[:, i:i + w] for i, t in enumerate(full_taps(taps)))


def column_sums(v, taps):
    """b(x, y): the tap-weighted sums of the row values down a column, border replicated, before the rounding"""
    R = len(taps) - 1
    q = np.pad(v, ((R, R), (0, 0)), mode="edge")
    h = v.shape[0]
    return sum(int(t) * q[i:i + h, :] for i, t in enumerate(full_taps(taps)))


def blur(plane, taps):
    """BLUR of a uint8 plane: the definition with np.pad"""
    v = (row_sums(plane, taps) + 64) >> 7
    return ((column_sums(v, taps) + (1 << 22)) >> 23).astype(np.uint8)


def blur_scipy(plane, taps):
    """BLUR of a uint8 plane: the definition with scipy.ndimage.correlate1d on int64"""
    from scipy import ndimage
    k = full_taps(taps)
    a = ndimage.correlate1d(np.asarray(plane).astype(np.int64), k, axis=1, mode="nearest")
    b = ndimage.correlate1d((a + 64) >> 7, k, axis=0, mode="nearest")
    return ((b + (1 << 22)) >> 23).astype(np.uint8)


def detail(plane, blurred):
    return np.clip(128 + np.asarray(plane).astype(np.int64) - blurred.astype(np.int64), 0, 255).astype(np.uint8)


def expected(src_planes, channels, taps, what, blur_of=blur):
    """the planes cvh_smooth_planes leaves in a destination of `channels` channels"""
    out, done = [], {}
    for k in range(channels):
        s = min(k, len(src_planes) - 1)
        p = np.array(src_planes[s], dtype=np.uint8)
        if what[k] == COPY:
            out.append(p)
            continue
        if s not in done:
            done[s] = blur_of(p, taps)
        out.append(done[s] if what[k] == BLUR else detail(p, done[s]))
    return out


@functools.lru_cache(maxsize=None)
def gauss_taps(sigma):
    """the header's formula for cvh_gauss_taps in numpy doubles: (R, tuple of R + 1 taps)"""
    R = int(math.ceil(3.0 * sigma))
    i = np.arange(R + 1, dtype=np.float64)
    e = np.exp(-(i * i) / (2.0 * sigma * sigma))
    S = e[0] + 2.0 * e[1:].sum()
    t = np.floor(32768.0 * e / S + 0.5).astype(np.int64)
    t[0] = TAP_SUM - 2 * int(t[1:].sum())
    return R, tuple(int(v) for v in t)


def box_taps(R):
    """a box of 2 R + 1 equal taps, the centre adjusted to the sum: at R = 3 all 4681 with a centre of 4682"""
    t = TAP_SUM // (2 * R + 1)
    return (TAP_SUM - 2 * R * t,) + (t,) * R


def kernel_of(name, R):
    """the tests' kernels at a radius: "gauss" (sigma = R / 3, whose radius is R), "box", and "rim": nearly all weight on the two
    outermost taps, nothing in between -- legal, and nothing like a decaying kernel"""
    if R == 0:
        return (TAP_SUM,)
    if name == "gauss":
        got, taps = gauss_taps(R / 3.0)
        assert got == R
        return taps
    if name == "box":
        return box_taps(R)
    assert name == "rim"
    return (2,) + (0,) * (R - 1) + (16383,)


def planes_of(kind, h, w, channels=1, seed=0):
    if kind == "all255":
        return [np.full((h, w), 255, np.uint8) for _ in range(channels)]
    return (blocky_planes if kind == "blocky" else random_planes)(h, w, channels, seed)


# The GPU cases: (h, w, R, kernel, kind).  One row more than a band and one column more than a strip of the column pass at R = 1 and at
# R = 63 (the band depends on the radius: 254 and 130 rows; it is never as short as a radius, so "a radius of one band" is the largest
# radius), and three bands at R = 63; a row and a column alone, where the clamp dominates; a window far wider than the plane; one column
# more than a row segment; the rim kernel and the box; the largest intermediates.
CASES = [(band_rows(1) + 1, STRIP + 1, 1, "gauss", "random"), (band_rows(1) + 1, STRIP + 1, 1, "rim", "blocky"),
         (band_rows(63) + 1, STRIP + 1, 63, "gauss", "random"), (band_rows(63) + 1, STRIP + 1, 63, "rim", "blocky"),
         (2 * band_rows(63) + 1, 2 * STRIP + 3, 63, "box", "blocky"),
         (1, 300, 20, "gauss", "random"), (300, 1, 20, "gauss", "random"), (1, 300, 63, "rim", "random"), (300, 1, 63, "rim", "random"),
         (5, 7, 63, "gauss", "random"), (5, 7, 63, "rim", "random"), (3, SEGMENT + 1, 5, "gauss", "random"), (2, SEGMENT + 7, 63, "rim", "blocky"),
         (33, 67, 3, "box", "blocky"), (33, 67, 0, "gauss", "random"), (70, 130, 63, "box", "all255"), None]
# A member has at most BLOCKS_MAX workgroups.  WIDE: 2 rows of 1025 strips are 130 row items and 1025 column items, so ONE workgroup of the
# column pass makes a second trip: the barrier in front of the tile's rewrite, the lane sums begun again, the flush into the 64-bit pair
BLOCKS_MAX = 1024
WIDE = (2, STRIP * BLOCKS_MAX + 1, 2, "gauss", "random")
CASES[-1] = WIDE
# 3 -> 3: 3 * 350 row items for those 1024 workgroups, so workgroups of the row pass make a second trip
LARGE = (350, 700, 63, "gauss", "random")
