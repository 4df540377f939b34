"""numpy / Python-integer restatement of the device-side initial level sets (include/chanvese_hip.h, "Device-side initial level sets"):
the grey sum, its histogram, Otsu's threshold as the header defines it, the three start arrays -- and an exact-rational Otsu for
cross-checking.  Shared by test_init_api.py (CPU) and test_gpu_init.py / test_gpu_torch_init.py / test_cli_init.py."""
from fractions import Fraction

import numpy as np

SHAPES = [(1, 1), (1, 23), (23, 1), (16, 16), (33, 47), (64, 144)]
KINDS = ["random", "flat", "two_valued", "all0", "all255", "ramp"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def grey(planes):
    """g(p) = sum_k I_k(p), 0 .. 255 C"""
    return np.sum([np.asarray(p, dtype=np.int64) for p in planes], axis=0)


def histogram(planes):
    return np.bincount(grey(planes).ravel(), minlength=255 * len(planes) + 1).astype(np.uint32)


def otsu_terms(hist):
    """[(t, d, q)] of every candidate t: exact Python integers"""
    h = [int(v) for v in hist]
    N, S = sum(h), sum(v * c for v, c in enumerate(h))
    out, n0, s0 = [], 0, 0
    for t in range(len(h) - 1):
        n0 += h[t]
        s0 += t * h[t]
        if 0 < n0 < N:
            out.append((t, S * n0 - N * s0, n0 * (N - n0)))
    return out


def otsu(hist):
    """the header's definition: the candidate with the largest float(d) * float(d) / float(q), ties to the smallest t; a single occupied
    bin v0 has no candidate and gives v0"""
    best, arg = -1.0, None
    for t, d, q in otsu_terms(hist):
        score = float(d) * float(d) / float(q)
        if score > best:
            best, arg = score, t
    if arg is None:
        occupied = np.flatnonzero(np.asarray(hist))
        assert occupied.size == 1, "an empty histogram has no threshold"
        return int(occupied[0])
    return arg


def otsu_exact(hist):
    """(t, score) maximising the exact rational d^2 / q, ties to the smallest t; (None, None) without a candidate"""
    best, arg = None, None
    for t, d, q in otsu_terms(hist):
        score = Fraction(d * d, q)
        if best is None or score > best:
            best, arg = score, t
    return arg, best


def exact_score(hist, t):
    for tt, d, q in otsu_terms(hist):
        if tt == t:
            return Fraction(d * d, q)
    return None


def start_threshold(planes, t, inside, outside):
    return np.where(grey(planes) > t, np.float64(inside), np.float64(outside))


def start_rect(h, w, x, y, rw, rh, inside, outside):
    rows, cols = np.mgrid[0:h, 0:w].astype(np.int64)
    m = (cols >= x) & (cols < x + rw) & (rows >= y) & (rows < y + rh)
    return np.where(m, np.float64(inside), np.float64(outside))


def start_disk(h, w, cx, cy, r, inside, outside):
    rows, cols = np.mgrid[0:h, 0:w].astype(np.int64)
    m = (cols - cx) ** 2 + (rows - cy) ** 2 <= int(r) ** 2
    return np.where(m, np.float64(inside), np.float64(outside))


def planes_of(kind, h, w, channels, seed=0):
    """the input cases: `channels` uint8 planes of h x w"""
    rng = np.random.default_rng(1000 * seed + 97 * h + 13 * w + channels)
    if kind == "random":
        return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(channels)]
    if kind == "flat":
        return [np.full((h, w), 37 + 50 * k, dtype=np.uint8) for k in range(channels)]
    if kind == "two_valued":
        m = rng.random((h, w)) < 0.3
        return [np.where(m, 200 - 10 * k, 20 + 5 * k).astype(np.uint8) for k in range(channels)]
    if kind == "all0":
        return [np.zeros((h, w), dtype=np.uint8) for _ in range(channels)]
    if kind == "all255":
        return [np.full((h, w), 255, dtype=np.uint8) for _ in range(channels)]
    if kind == "ramp":
        # grey value p mod B at pixel p: every bin is occupied once the plane has B pixels; channel k takes what the ones before left
        g = (np.arange(h * w, dtype=np.int64) % (255 * channels + 1)).reshape(h, w)
        out = []
        for _ in range(channels):
            out.append(np.minimum(g, 255).astype(np.uint8))
            g = g - out[-1]
        return out
    raise ValueError(kind)


def histograms_for_otsu(seed=0):
    """name -> histogram (uint32): random and structured ones, 256 and 766 bins"""
    rng = np.random.default_rng(seed)
    out = {}
    for B in (256, 766):
        out[f"uniform random {B}"] = rng.integers(0, 1000, B).astype(np.uint32)
        sparse = np.zeros(B, dtype=np.uint32)
        sparse[rng.choice(B, 7, replace=False)] = rng.integers(1, 50, 7)
        out[f"sparse {B}"] = sparse
        x = np.arange(B)
        out[f"bimodal {B}"] = (900 * np.exp(-((x - B * 0.25) / (B * 0.05)) ** 2) + 400 * np.exp(-((x - B * 0.7) / (B * 0.1)) ** 2)).astype(np.uint32)
        two = np.zeros(B, dtype=np.uint32)
        two[3], two[B - 2] = 10, 1
        out[f"two bins {B}"] = two
        out[f"all ones {B}"] = np.ones(B, dtype=np.uint32)
        big = rng.integers(0, 1 << 20, B).astype(np.uint32)
        out[f"large counts {B}"] = big
    return out


def huge_histograms():
    """766 bins with counts near 2^31 in two or three of them: d = S n0 - N s0 passes 2^64"""
    out = {}
    for name, bins in (("two far", {1: 2 ** 31 - 1, 764: 2 ** 31 - 3}), ("three", {0: 2 ** 31 - 1, 400: 2 ** 31 - 7, 765: 2 ** 31 - 2}),
                       ("three near", {700: 2 ** 31 + 5, 701: 2 ** 31 - 1, 765: 2 ** 32 - 1}), ("two near the top", {762: 2 ** 32 - 1, 765: 2 ** 32 - 1})):
        h = np.zeros(766, dtype=np.uint32)
        for v, c in bins.items():
            h[v] = c
        out[name] = h
    return out


def degenerate_histograms():
    """name -> (histogram, t): ties (the smallest t wins), a single occupied bin, bin 0 only, bin B-1 only"""
    out = {}
    for B in (256, 766):
        h = np.zeros(B, dtype=np.uint32); h[10] = h[20] = 5
        out[f"tie plateau {B}"] = (h, 10)            # every t in 10 .. 19 splits the same way
        h = np.zeros(B, dtype=np.uint32); h[0] = h[B - 1] = 1
        out[f"ends {B}"] = (h, 0)
        h = np.zeros(B, dtype=np.uint32); h[B // 2] = 9
        out[f"single bin {B}"] = (h, B // 2)
        h = np.zeros(B, dtype=np.uint32); h[0] = 4
        out[f"bin 0 only {B}"] = (h, 0)
        h = np.zeros(B, dtype=np.uint32); h[B - 1] = 4
        out[f"bin B-1 only {B}"] = (h, B - 1)
    return out
