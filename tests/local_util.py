"""Restatements of the local-statistics calls (include/chanvese_hip.h, "Local statistics"), the cases the tests share, and the
proposition's image with its runs on the CPU oracle.  Two independent restatements of the header's integer definition: a window loop
in Python integers (small planes), and summed-area tables in int64 with math.isqrt.  The definition is in integers, so every comparison
against it is an equality.  Shared by test_local_restatement.py, test_local_api.py (CPU), test_gpu_local.py, test_gpu_torch_local.py
and test_cli_local.py."""
import functools
import math

import numpy as np

COPY, MEAN, DEV = 0, 1, 2
RADIUS_MAX = 127
STACK = (COPY, MEAN, DEV)
# local_kernels.hip: a wave of the column pass takes BAND rows x STRIP columns per trip, a workgroup of the row pass SEGMENT columns of
# a row (cvh_internal.h, CVH_WINDOW_*; test_local_api.py compares these numbers with the library's)
BAND, STRIP, SEGMENT = 32, 256, 1024

_ISQRT = np.array([math.isqrt(q) for q in range(255 * 255 + 1)], dtype=np.int64)


def brute(plane, R):
    """(MEAN, DEV) of a uint8 plane, pixel by pixel in Python integers: the definition as written"""
    h, w = plane.shape
    p = [[int(v) for v in row] for row in plane]
    mean, dev = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    for r in range(h):
        for c in range(w):
            win = [p[i][j] for i in range(max(r - R, 0), min(r + R, h - 1) + 1) for j in range(max(c - R, 0), min(c + R, w - 1) + 1)]
            n, S, Q = len(win), sum(win), sum(v * v for v in win)
            mean[r, c] = (2 * S + n) // (2 * n)
            dev[r, c] = math.isqrt(4 * (n * Q - S * S) // (n * n))
    return mean, dev


def window_sums(plane, R):
    """(n, S, Q) per pixel, int64, from summed-area tables"""
    h, w = plane.shape
    p = plane.astype(np.int64)
    r0, r1 = np.maximum(np.arange(h) - R, 0), np.minimum(np.arange(h) + R, h - 1) + 1
    c0, c1 = np.maximum(np.arange(w) - R, 0), np.minimum(np.arange(w) + R, w - 1) + 1

    def box(a):
        t = np.zeros((h + 1, w + 1), np.int64)
        t[1:, 1:] = a.cumsum(0).cumsum(1)
        return t[r1][:, c1] - t[r0][:, c1] - t[r1][:, c0] + t[r0][:, c0]

    return (r1 - r0)[:, None] * (c1 - c0)[None, :], box(p), box(p * p)


def fast(plane, R):
    """(MEAN, DEV) of a uint8 plane from summed-area tables"""
    n, S, Q = window_sums(plane, R)
    q = 4 * (n * Q - S * S) // (n * n)
    assert q.min() >= 0 and q.max() <= 255 * 255
    return ((2 * S + n) // (2 * n)).astype(np.uint8), _ISQRT[q].astype(np.uint8)


def expected(src_planes, channels, R, what, stats=fast):
    """the planes cvh_local_planes leaves in a destination of `channels` channels"""
    out, done = [], {}
    for k in range(channels):
        s = min(k, len(src_planes) - 1)
        if what[k] == COPY:
            out.append(np.array(src_planes[s], dtype=np.uint8))
            continue
        if s not in done:
            done[s] = stats(np.asarray(src_planes[s]), R)
        out.append(done[s][what[k] - 1])
    return out


def random_planes(h, w, channels=1, seed=0):
    from chan_vese_amd import synth
    z = synth.splitmix64_stream(100003 * h + 101 * w + seed, channels * h * w)
    return [(z[k * h * w:(k + 1) * h * w] >> np.uint64(56)).astype(np.uint8).reshape(h, w) for k in range(channels)]


def blocky_planes(h, w, channels=1, seed=0):
    """random bytes in 5 x 3 blocks of one value plus low noise: windows of every mix of flat and busy"""
    out = []
    for k, z in enumerate(random_planes((h + 4) // 5, (w + 2) // 3, channels, seed + 7)):
        big = np.repeat(np.repeat(z, 5, axis=0), 3, axis=1)[:h, :w].astype(np.int64)
        out.append(np.clip(big + (random_planes(h, w, 1, seed + 11 + k)[0] & 7), 0, 255).astype(np.uint8))
    return out


# small planes for the window loop: (h, w, R)
SMALL = [(1, 1, 0), (1, 1, 3), (1, 9, 2), (9, 1, 2), (5, 7, 0), (5, 7, 1), (5, 7, 127), (8, 8, 3), (7, 12, 4), (13, 11, 6)]

# The GPU cases: (h, w, R, kind).  A row and a column alone; the window is the whole plane at every pixel; odd sizes with tails narrower
# than a 16-byte piece and than a lane's four columns; one row more than a band and one column more than a strip, with a small radius and
# with R = the band height (a window taller than a band); one column more than a row segment, with a span that crosses the seam at both
# radii; full 255 x 255 windows next to windows truncated on two sides; the largest intermediates.
CASES = [(1, 40, 3, "random"), (40, 1, 3, "random"), (5, 7, 127, "random"), (33, 67, 1, "random"), (33, 67, 5, "blocky"),
         (BAND + 1, STRIP + 1, 2, "random"), (BAND + 1, STRIP + 1, BAND, "blocky"), (3, SEGMENT + 1, 5, "random"), (2, SEGMENT + 7, 127, "blocky"),
         (300, 260, 127, "random"), (256, 256, 127, "all255")]
LARGE = (1024, 1536, 3, "random")     # many workgroups; the row pass makes a second trip


def planes_of(kind, h, w, channels=1, seed=0):
    if kind == "all255":
        return [np.full((h, w), 255, np.uint8) for _ in range(channels)]
    return (blocky_planes if kind == "blocky" else random_planes)(h, w, channels, seed)


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    union = (a | b).sum()
    return 1.0 if union == 0 else (a & b).sum() / union


def iou_either(a, b):
    """polarity-agnostic: a checkerboard start can converge to either sign"""
    return max(iou(a, b), iou(a, 1 - (np.asarray(b) != 0)))


# ---- the proposition: a disk whose MEAN is the ground's and whose noise is four times as wide.  On the raw plane the run has nothing to
# separate; on the local deviation plane it finds the disk.
PROP_N, PROP_SEED, PROP_R = 128, 7, 2


def proposition_truth(n=PROP_N):
    ii = np.arange(n, dtype=np.int64)[:, None] - n // 2
    jj = np.arange(n, dtype=np.int64)[None, :] - n // 2
    return (ii * ii + jj * jj <= (n // 4) ** 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def proposition_image(n=PROP_N, seed=PROP_SEED):
    """One uint8 plane, integers only: 128 + noise, clipped; the noise is the sum of four uniform integers of -a .. a from
    synth.splitmix64_stream, a = 20 inside the disk and 5 outside.  Shared, do not modify."""
    from chan_vese_amd import synth
    a = np.where(proposition_truth(n) != 0, 20, 5).astype(np.int64)
    z = synth.splitmix64_stream(seed, 4 * n * n).reshape(4, n, n)
    noise = sum((z[t] % (2 * a + 1).astype(np.uint64)).astype(np.int64) - a for t in range(4))
    p = np.clip(128 + noise, 0, 255).astype(np.uint8)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def proposition_plane(kind, R=PROP_R):
    """the plane a row of the table iterates on: "raw", or "dev" at radius R.  Shared, do not modify."""
    p = proposition_image() if kind == "raw" else fast(proposition_image(), R)[1]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def oracle_proposition(kind, R=PROP_R):
    """The CPU oracle on the proposition's plane: checkerboard start, default parameters, 600 steps at most.  Returns (u, steps, IoU
    with the disk).  Computed once per process; do not modify."""
    from oracle import cv_oracle as O
    n = PROP_N
    u, steps, _, _ = O.csv_run([np.array(proposition_plane(kind, R))], O.checkerboard(n, n), O.make_params(), 600, trace=False)
    u.setflags(write=False)
    return u, steps, iou_either(proposition_truth(n), O.mask(u))
