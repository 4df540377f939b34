"""Restatements of the rank-plane calls (include/chanvese_hip.h, "Rank planes"), the cases the tests share, and the two propositions'
images with their runs on the CPU oracle.  Two independent restatements of the header's definition: a window loop in Python integers
with `sorted` (small planes), and a fast one -- running extrema along rows then columns for MIN and MAX, sorted sliding windows padded
with a sentinel of 256 for the median.  The definition is in integers, so every comparison against it is an equality.  Shared by
test_rank_restatement.py, test_rank_api.py, test_cli_rank.py (CPU), test_gpu_rank.py and test_gpu_torch_rank.py."""
import functools

import numpy as np

import local_util as L

COPY, MIN, MAX, MEDIAN, OPEN, CLOSE, TOPHAT, BOTHAT = range(8)
CODES = (COPY, MIN, MAX, MEDIAN, OPEN, CLOSE, TOPHAT, BOTHAT)
NAMES = {"min": MIN, "max": MAX, "median": MEDIAN, "open": OPEN, "close": CLOSE, "tophat": TOPHAT, "bothat": BOTHAT}
RADIUS_MAX, MEDIAN_RADIUS_MAX = 127, 7
# rank_kernels.hip: a wave of the column passes takes band_rows(R) rows x STRIP columns per trip, a workgroup of the row pass SEGMENT
# columns of a row, a wave of the median MEDIAN_BAND rows x MEDIAN_STRIP columns (cvh_internal.h, CVH_WINDOW_* and CVH_RANK_MEDIAN_*; test_rank_api.py compares
# these numbers with the library's)
BAND, STRIP, SEGMENT, MEDIAN_BAND, MEDIAN_STRIP = 32, 256, 1024, 32, 64


def band_rows(R):
    """rows of a column band at radius R: the least multiple of the van Herk block 2 R + 1 that is not below BAND"""
    K = 2 * R + 1
    return K * ((BAND + K - 1) // K)


# ---- the first restatement: the definition as written

def _windows(plane, R):
    h, w = plane.shape
    p = [[int(v) for v in row] for row in plane]
    for r in range(h):
        for c in range(w):
            yield r, c, sorted(p[i][j] for i in range(max(r - R, 0), min(r + R, h - 1) + 1) for j in range(max(c - R, 0), min(c + R, w - 1) + 1))


def brute_one(plane, R, pick):
    out = np.zeros(plane.shape, np.uint8)
    for r, c, s in _windows(plane, R):
        out[r, c] = pick(s)
    return out


def brute(plane, R, code):
    """one code of a uint8 plane, pixel by pixel in Python integers with sorted()"""
    plane = np.asarray(plane, dtype=np.uint8)
    lo, hi = (lambda s: s[0]), (lambda s: s[-1])
    if code == COPY:
        return plane.copy()
    if code == MIN:
        return brute_one(plane, R, lo)
    if code == MAX:
        return brute_one(plane, R, hi)
    if code == MEDIAN:
        return brute_one(plane, R, lambda s: s[(len(s) - 1) // 2])
    if code in (OPEN, TOPHAT):
        opened = brute_one(brute_one(plane, R, lo), R, hi)
        return opened if code == OPEN else (plane.astype(np.int64) - opened).astype(np.uint8)
    if code in (CLOSE, BOTHAT):
        closed = brute_one(brute_one(plane, R, hi), R, lo)
        return closed if code == CLOSE else (closed.astype(np.int64) - plane).astype(np.uint8)
    raise ValueError(code)


# ---- the second restatement: fast

def _running(a, R, axis, op):
    """op over the truncated window of radius R along one axis: the accumulate of op over the 2 R + 1 shifts that stay inside"""
    n = a.shape[axis]
    out = a.copy()
    for d in range(1, min(R, n - 1) + 1):
        src_lo, dst_lo = [slice(None)] * 2, [slice(None)] * 2
        src_lo[axis], dst_lo[axis] = slice(d, None), slice(0, n - d)          # element i sees i + d
        out[tuple(dst_lo)] = op(out[tuple(dst_lo)], a[tuple(src_lo)])
        src_lo[axis], dst_lo[axis] = slice(0, n - d), slice(d, None)          # element i sees i - d
        out[tuple(dst_lo)] = op(out[tuple(dst_lo)], a[tuple(src_lo)])
    return out


def _extreme(plane, R, op):
    if R >= 16:                                                               # (the shifts below cost 2 R passes over the plane)
        try:
            from scipy import ndimage
            f = ndimage.minimum_filter if op is np.minimum else ndimage.maximum_filter
            return f(plane, size=2 * R + 1, mode="nearest")                   # equals the truncated window for an extremum
        except ImportError:
            pass
    return _running(_running(plane, R, 1, op), R, 0, op)


def fast_min(plane, R):
    return _extreme(np.asarray(plane, dtype=np.uint8), R, np.minimum)


def fast_max(plane, R):
    return _extreme(np.asarray(plane, dtype=np.uint8), R, np.maximum)


def fast_median(plane, R, chunk_rows=64):
    """sliding windows over the plane padded with the sentinel 256 (int16), sorted; element (n - 1) // 2 per pixel, in row chunks"""
    plane = np.asarray(plane, dtype=np.uint8)
    h, w = plane.shape
    if R == 0:
        return plane.copy()
    K = 2 * R + 1
    padded = np.full((h + 2 * R, w + 2 * R), 256, np.int16)
    padded[R:R + h, R:R + w] = plane
    nr = np.minimum(np.arange(h) + R, h - 1) - np.maximum(np.arange(h) - R, 0) + 1
    nc = np.minimum(np.arange(w) + R, w - 1) - np.maximum(np.arange(w) - R, 0) + 1
    out = np.empty((h, w), np.uint8)
    for r0 in range(0, h, chunk_rows):
        r1 = min(r0 + chunk_rows, h)
        win = np.lib.stride_tricks.sliding_window_view(padded[r0:r1 + 2 * R], (K, K)).reshape(r1 - r0, w, K * K)
        srt = np.sort(win, axis=2)
        idx = (nr[r0:r1, None] * nc[None, :] - 1) // 2
        got = np.take_along_axis(srt, idx[:, :, None], axis=2)[:, :, 0]
        assert got.max() <= 255
        out[r0:r1] = got
    return out


def fast(plane, R, code):
    """one code of a uint8 plane, the fast way"""
    plane = np.asarray(plane, dtype=np.uint8)
    if code == COPY:
        return plane.copy()
    if code == MIN:
        return fast_min(plane, R)
    if code == MAX:
        return fast_max(plane, R)
    if code == MEDIAN:
        return fast_median(plane, R)
    if code in (OPEN, TOPHAT):
        opened = fast_max(fast_min(plane, R), R)
        return opened if code == OPEN else (plane.astype(np.int16) - opened).astype(np.uint8)
    if code in (CLOSE, BOTHAT):
        closed = fast_min(fast_max(plane, R), R)
        return closed if code == CLOSE else (closed.astype(np.int16) - plane).astype(np.uint8)
    raise ValueError(code)


def expected(src_planes, channels, R, what, one=fast):
    """the planes cvh_rank_planes leaves in a destination of `channels` channels"""
    done = {}
    out = []
    for k in range(channels):
        s = min(k, len(src_planes) - 1)
        if (s, what[k]) not in done:
            done[s, what[k]] = one(np.asarray(src_planes[s]), R, what[k])
        out.append(done[s, what[k]])
    return out


random_planes, blocky_planes, planes_of = L.random_planes, L.blocky_planes, L.planes_of
iou, iou_either = L.iou, L.iou_either


def zero_planes(h, w, channels=1):
    return [np.zeros((h, w), np.uint8) for _ in range(channels)]


def split_planes(h, w, channels=1):
    """half 0 and half 255, split by a vertical line: the median's rank sits on the bin boundary"""
    p = np.zeros((h, w), np.uint8)
    p[:, w // 2:] = 255
    return [p.copy() for _ in range(channels)]


# small planes for the window loop: local_util.SMALL's shapes, with the radius cut to 7 where the median is taken
SMALL = L.SMALL

# The GPU cases of the separable codes: (h, w, R, kind).  A row and a column alone; the window is the whole plane at every pixel; odd
# sizes with tails narrower than a lane's four columns; one row more than a band and one column more than a strip, at R = 2 and R = the
# band height; one column more than a row segment with a van Herk block that straddles the seam; a plane narrower and shorter than one
# block; a width that is an exact multiple of 2 R + 1 and one more than that.
CASES = [(1, 40, 3, "random"), (40, 1, 3, "random"), (5, 7, 127, "random"), (33, 67, 1, "random"), (33, 67, 2, "blocky"), (33, 67, 3, "random"),
         (33, 67, 7, "blocky"), (BAND + 1, STRIP + 1, 2, "random"), (BAND + 1, STRIP + 1, BAND, "blocky"), (band_rows(2) + 1, STRIP + 1, 2, "blocky"),
         (3, SEGMENT + 1, 5, "random"), (2, SEGMENT + 7, 127, "blocky"), (9, 11, 127, "random"), (20, 7 * 11, 5, "random"), (20, 7 * 11 + 1, 5, "blocky"),
         (70, 30, 0, "random"), (256, 64, 127, "all255")]
# the median's: every R on (33, 67), the whole plane as window, R = 7 across the band and strip seams
MEDIAN_CASES = [(33, 67, R, "random") for R in range(8)] + [(5, 7, 7, "random"), (1, 40, 3, "random"), (40, 1, 3, "blocky"),
                                                             (MEDIAN_BAND + 1, STRIP + 1, 7, "blocky"), (MEDIAN_BAND + 1, STRIP + 1, 2, "random"),
                                                             (33, 67, 7, "all255"), (33, 67, 7, "zero"), (33, 67, 7, "split"), (20, 40, 3, "split")]
LARGE = (1024, 1536, 3, "random")     # many workgroups; the row pass and the median make a second trip


def case_planes(kind, h, w, channels=1, seed=0):
    if kind == "zero":
        return zero_planes(h, w, channels)
    if kind == "split":
        return split_planes(h, w, channels)
    return planes_of(kind, h, w, channels, seed)


# ---- the two propositions.  Shared, do not modify.
PROP_N, PROP_SEED = 128, 11
SALT_R, RAMP_R = 2, 10
RAMP_CENTRES = ((24, 24), (24, 100), (64, 60), (100, 30), (104, 104), (60, 110), (40, 64))


@functools.lru_cache(maxsize=None)
def _streams():
    from chan_vese_amd import synth
    return synth.splitmix64_stream(PROP_SEED, 2 * PROP_N * PROP_N).reshape(2, PROP_N, PROP_N)


def salt_truth():
    """the disk ii^2 + jj^2 <= 32^2 about (64, 64).  Shared, do not modify."""
    ii = np.arange(PROP_N, dtype=np.int64)[:, None] - 64
    jj = np.arange(PROP_N, dtype=np.int64)[None, :] - 64
    return (ii * ii + jj * jj <= 32 * 32).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def salt_image():
    """150 inside the disk and 100 outside; sel = z[0] % 100: sel < 15 a 0, 15 <= sel < 30 a 255.  Shared, do not modify."""
    base = np.where(salt_truth() != 0, 150, 100).astype(np.int64)
    sel = (_streams()[0] % np.uint64(100)).astype(np.int64)
    p = np.where(sel < 15, 0, np.where(sel < 30, 255, base)).astype(np.uint8)
    p.setflags(write=False)
    return p


def ramp_truth():
    """the union of seven disks of radius 8.  Shared, do not modify."""
    ii = np.arange(PROP_N, dtype=np.int64)[:, None]
    jj = np.arange(PROP_N, dtype=np.int64)[None, :]
    t = np.zeros((PROP_N, PROP_N), bool)
    for r, c in RAMP_CENTRES:
        t |= (ii - r) ** 2 + (jj - c) ** 2 <= 8 * 8
    return t.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def ramp_image():
    """p = clip(40 + (col * 140) // 127 + 40 * truth + (z[1] % 9 - 4), 0, 255).  Shared, do not modify."""
    col = np.arange(PROP_N, dtype=np.int64)[None, :]
    noise = (_streams()[1] % np.uint64(9)).astype(np.int64) - 4
    p = np.clip(40 + (col * 140) // 127 + 40 * ramp_truth().astype(np.int64) + noise, 0, 255).astype(np.uint8)
    p.setflags(write=False)
    return p


# the rows of the two tables: name -> (image, code, R, truth)
PROPOSITIONS = {"salt raw": (salt_image, COPY, 0, salt_truth), "salt median R=1": (salt_image, MEDIAN, 1, salt_truth),
                "salt median R=2": (salt_image, MEDIAN, SALT_R, salt_truth), "ramp raw": (ramp_image, COPY, 0, ramp_truth),
                "ramp tophat R=10": (ramp_image, TOPHAT, RAMP_R, ramp_truth)}


@functools.lru_cache(maxsize=None)
def proposition_plane(name):
    """the plane a row of the tables iterates on.  Shared, do not modify."""
    image, code, R, _ = PROPOSITIONS[name]
    p = fast(np.array(image()), R, code)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def oracle_proposition(name):
    """The CPU oracle on a row's plane: checkerboard start, default parameters, 600 steps at most.  Returns (u, steps, IoU with the
    truth, the better of the mask and its inverse).  Computed once per process; do not modify."""
    from oracle import cv_oracle as O
    n = PROP_N
    u, steps, _, _ = O.csv_run([np.array(proposition_plane(name))], O.checkerboard(n, n), O.make_params(), 600, trace=False)
    u.setflags(write=False)
    return u, steps, iou_either(PROPOSITIONS[name][3](), O.mask(u))
