"""The localised Chan-Vese iteration of include/chanvese_hip.h, "Localised regions", restated in numpy on np_restatement's heaviside /
delta / curvature / combine_folded -- what the device is compared against (test_gpu_localized.py) and what the CPU tests state facts
about (test_localized_restatement.py) -- with the cases, the demonstration scene and the perturbation bound the GPU tolerance is.

Window sums are exact uint64 integers taken with 2-D cumulative sums.  The cumulative sums may wrap modulo 2^64 on a large plane; the
four-corner difference is still exact because the true window sum is below 2^64 (65025 * 255 * 2^40)."""
import functools
import math

import numpy as np

import np_restatement as R

FRAC_BITS = 40
ONE = 1 << FRAC_BITS
RADIUS_MAX = 127
COLS = 61            # output columns per wave of the step kernel
SEGMENT = 1024       # columns per workgroup trip of the row pass (CVH_WINDOW_SEGMENT)
ITERATIONS = 6

DEFAULT = dict(mu=0.5, nu=0.0, dt=1.0, eps=1.0, tol=0.0, lambda1=(1.0, 1.0, 1.0), lambda2=(1.0, 1.0, 1.0))
OTHER = dict(mu=0.3, nu=0.05, dt=0.7, eps=1.0, tol=0.0, lambda1=(1.2, 0.9, 1.1), lambda2=(0.8, 1.1, 1.0))


def box_sums(x, rad):
    """sum of x over the (2 rad + 1)^2 window truncated at the border, uint64, by 2-D cumulative sums"""
    x = np.asarray(x, dtype=np.uint64)
    h, w = x.shape
    cs = np.zeros((h + 1, w + 1), dtype=np.uint64)
    cs[1:, 1:] = np.cumsum(np.cumsum(x, axis=0, dtype=np.uint64), axis=1, dtype=np.uint64)
    r0, r1 = np.maximum(np.arange(h) - rad, 0), np.minimum(np.arange(h) + rad, h - 1) + 1
    c0, c1 = np.maximum(np.arange(w) - rad, 0), np.minimum(np.arange(w) + rad, w - 1) + 1
    return cs[r1][:, c1] - cs[r0][:, c1] - cs[r1][:, c0] + cs[r0][:, c0]


def box_sums_brute(x, rad):
    """the same by a double loop in Python integers"""
    h, w = x.shape
    out = np.zeros((h, w), dtype=object)
    xi = [[int(v) for v in row] for row in x]
    for r in range(h):
        for c in range(w):
            out[r, c] = sum(xi[j][i] for j in range(max(r - rad, 0), min(r + rad, h - 1) + 1) for i in range(max(c - rad, 0), min(c + rad, w - 1) + 1))
    return out


def window_counts(h, w, rad):
    nr = np.minimum(np.arange(h) + rad, h - 1) - np.maximum(np.arange(h) - rad, 0) + 1
    nc = np.minimum(np.arange(w) + rad, w - 1) - np.maximum(np.arange(w) - rad, 0) + 1
    return (nr[:, None] * nc[None, :]).astype(np.uint64)


def weights(u, eps=1.0, factor=None):
    """wq = rint(H_eps(u) 2^40) in [0, 2^40]; factor: a per-pixel multiplier of H_eps (the perturbation bound's)"""
    H = R.heaviside(u, eps)
    if factor is not None:
        H = H * factor
    return np.clip(np.rint(H * float(ONE)), 0.0, float(ONE)).astype(np.uint64)


def sums_of(planes, wq, rad):
    """(A, [S_k]) of the weights wq"""
    return box_sums(wq, rad), [box_sums(wq * p.astype(np.uint64), rad) for p in planes]


def means_of(planes, wq, rad):
    """(c1[k], c2[k], A, S[k]) as the header defines them: one conversion each, one division"""
    h, w = wq.shape
    A, S = sums_of(planes, wq, rad)
    B = window_counts(h, w, rad) * np.uint64(ONE) - A
    c1, c2 = [], []
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, p in enumerate(planes):
            T = box_sums(p, rad)
            Sp = T * np.uint64(ONE) - S[k]
            c1.append(S[k].astype(np.float64) / A.astype(np.float64))
            c2.append(Sp.astype(np.float64) / B.astype(np.float64))
    return c1, c2, A, S


def step(planes, u, p, rad, factor=None):
    """one iteration: (new u, ||d||)"""
    C = len(planes)
    c1, c2, _, _ = means_of(planes, weights(u, p["eps"], factor), rad)
    F = np.zeros_like(u)
    for k, img in enumerate(planes):
        f = img.astype(np.float64)
        F += -p["lambda1"][k] * (f - c1[k]) ** 2 + p["lambda2"][k] * (f - c2[k]) ** 2
    d = R.combine_folded(R.curvature(u), F, p["mu"], p["nu"], p["dt"], C) * R.delta(u, p["eps"])
    return u + d, math.sqrt(float(np.sum(d * d)))


def run(planes, u, p, rad, max_steps, stop=None, factors=None):
    """cvh_localized_run: (u, steps_done, trace) -- a trace row is ||d||"""
    if stop is None:
        stop = R.stop_condition(planes, p["tol"])
    rows = []
    for t in range(max_steps):
        u, nrm = step(planes, u, p, rad, None if factors is None else factors[t])
        rows.append(nrm)
        if nrm <= stop:
            break
    return u, len(rows), np.array(rows)


def global_run(planes, u, p, max_steps):
    """the two-phase model from the same start (np_restatement.csv_step): the demonstration's other side"""
    for _ in range(max_steps):
        u = R.csv_step(planes, u, p["mu"], p["nu"], p["dt"], p["eps"], p["lambda1"][:len(planes)], p["lambda2"][:len(planes)])[0]
    return u


def mask(u):
    """cvh_get_mask(invert = 0): (float)u > 0"""
    return (u.astype(np.float32) > 0).astype(np.uint8)


def iou(a, b):
    a, b = a.astype(bool), b.astype(bool)
    return float((a & b).sum()) / float((a | b).sum())


# ---- the partition (cvh_loc_geometry, localized_kernels.hip), restated so that the cases exist without the library;
# test_localized_api.py holds the library to it
def geometry(h, w, rad):
    """(cols, item_rows, items, strip_rows)"""
    nwc = -(-w // COLS)
    target = max(4096 // nwc, 1)
    item_rows = max((-(-h // target) + 3) & ~3, 8)
    nitem_rows = -(-h // item_rows)
    lead = 2 * (2 * rad + 1)
    strip_rows = min(item_rows * -(-lead // item_rows), item_rows * nitem_rows)
    return COLS, item_rows, nitem_rows * nwc, strip_rows


# ---- images and starts
def scene(h, w, channels=1, seed=5):
    """a disk of +50 grey on a horizontal ramp 40 .. 190 (channel k: the ramp reversed for odd k), Gaussian noise sigma 3"""
    yy, xx = np.mgrid[0:h, 0:w]
    rad = 0.3 * max(min(h, w), 2)
    disk = (xx - (w - 1) / 2.0) ** 2 + (yy - (h - 1) / 2.0) ** 2 <= rad ** 2
    rng = np.random.default_rng(seed)
    planes = []
    for k in range(channels):
        ramp = 40.0 + 150.0 * (xx / max(w - 1, 1))
        if k & 1:
            ramp = ramp[:, ::-1]
        g = ramp + 50.0 * disk + rng.normal(0.0, 3.0, (h, w))
        planes.append(np.clip(np.rint(g), 0, 255).astype(np.uint8))
    return planes, disk


def start(h, w):
    """a smooth start with a front inside every shape: the signed distance to a centred disk, scaled so that H_eps stays well inside
    (0, 1) over the plane -- the sums are then well conditioned"""
    yy, xx = np.mgrid[0:h, 0:w]
    rad = 0.32 * max(min(h, w), 2)
    sd = rad - np.sqrt((xx - (w - 1) / 2.0) ** 2 + (yy - (h - 1) / 2.0) ** 2)
    return np.clip(sd, -3.0, 3.0) + 0.0


SEAM_R = 1
SEAM_H = geometry(1, 130, SEAM_R)[3] + 1     # one row past the strip a short plane of 130 columns gets at R = 1
assert geometry(SEAM_H, 130, SEAM_R)[3] == SEAM_H - 1
ITEM_R = 5                                    # a strip of several items: the item seams inside it, and one row past it
ITEM_H = geometry(1000, 70, ITEM_R)[3] + 1   # (the strip of a plane tall enough not to cap it; still 8-row items)
assert geometry(ITEM_H, 70, ITEM_R)[1] < geometry(ITEM_H, 70, ITEM_R)[3] == ITEM_H - 1

# (h, w, channels, radius, parameter set)
CASES = [
    # windows larger than the plane; nu != 0 there
    (1, 7, 1, 1, "other"), (1, 7, 1, 127, "other"), (7, 1, 1, 1, "other"), (7, 1, 1, 127, "other"), (2, 2, 1, 1, "other"), (2, 2, 1, 127, "other"),
    # one wave column, one lane past it, two columns of the step kernel
    (5, COLS, 1, 2, "default"), (6, COLS + 1, 1, 2, "default"), (9, 2 * COLS, 1, 3, "other"),
    # one row past a strip; a strip of three items and one row past it
    (SEAM_H, 130, 1, SEAM_R, "default"), (ITEM_H, 70, 1, ITEM_R, "other"),
    # a row segment seam of the row pass
    (3, SEGMENT - 1, 1, 2, "default"), (3, SEGMENT, 1, 2, "default"), (3, SEGMENT + 1, 1, 4, "default"),
    # the largest radius on thin planes
    (9, 300, 1, 127, "default"), (300, 9, 1, 127, "default"),
    # three channels, non-default lambda
    (67, 65, 3, 6, "other"), (67, 65, 3, 10, "default"),
]


def case_id(case):
    h, w, C, rad, which = case
    return f"{h}x{w}x{C}-R{rad}-{which}"


def params_of(which):
    return DEFAULT if which == "default" else OTHER


@functools.lru_cache(maxsize=None)
def case_inputs(h, w, C):
    planes, _ = scene(h, w, C)
    u = start(h, w)
    for a in planes + [u]:
        a.setflags(write=False)
    return planes, u


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """the restatement's run of a case: computed once, shared, read-only"""
    h, w, C, rad, which = case
    planes, u = case_inputs(h, w, C)
    v, steps, trace = run(planes, u, params_of(which), rad, ITERATIONS)
    v.setflags(write=False)
    trace.setflags(write=False)
    return v, steps, trace


# ---- the perturbation bound
ULP = 2.0 ** -52


def perturbed_distance(case, seed=20):
    """max |u - u'| after the case's iterations, u' run with H_eps multiplied by (1 +- 2 ulp) at random per pixel and iteration: what a
    device atan within 2 ulp, or a FAST form of H_eps, may do to the result"""
    h, w, C, rad, which = case
    planes, u = case_inputs(h, w, C)
    rng = np.random.default_rng(seed)
    factors = [1.0 + 2.0 * ULP * rng.choice([-1.0, 1.0], size=(h, w)) for _ in range(ITERATIONS)]
    v = run(planes, u, params_of(which), rad, ITERATIONS, factors=factors)[0]
    return float(np.abs(v - case_reference(case)[0]).max())


@functools.lru_cache(maxsize=None)
def tolerance():
    """the GPU tolerance on u: ten times the largest perturbed distance over the cases (one decimal of margin for forms not modelled:
    the refined reciprocals and square roots of CVH_MATH_FAST, the device's division)"""
    return 10.0 * max(perturbed_distance(c) for c in CASES)


def trace_tolerance(h, w):
    """on ||d||: d = u(t+1) - u(t), so |d - d'| <= 2 tolerance() per pixel and | ||d|| - ||d'|| | <= ||d - d'|| <= 2 tolerance() sqrt(h w)"""
    return 2.0 * tolerance() * math.sqrt(h * w)


# ---- the demonstration (the issue's scene): 64^2, disk of +50 on a ramp 40 .. 190, sigma 3, seed 3; start: signed distance to a disk
# of radius 0.32 * 64 at the centre; 300 iterations, tol 0
# The disk's own radius is not part of that description; 0.18 * 64 is taken here.  Measured with this restatement (IoU with the disk):
# localised R = 10, mu = 100: 0.995; R = 6, mu = 100: 0.814; R = 6, mu = 0.5: 0.478; global model, default parameters: 0.192 (it cuts
# the ramp in two).  The model's own limit shows on a larger disk: at radius 0.25 * 64 the disk itself is found exactly by R = 6
# (1.000) and by R = 10, but with R = 10 spurious regions grow along the left and right borders, far from the front, where the force
# is noise (IoU 0.651 after 300 iterations, 0.906 after 50).
DEMO_N, DEMO_STEPS, DEMO_DISK = 64, 300, 0.18
DEMO_LOCAL = dict(DEFAULT, mu=100.0)
DEMO_RADIUS = 10


@functools.lru_cache(maxsize=None)
def demo_inputs():
    n = DEMO_N
    yy, xx = np.mgrid[0:n, 0:n]
    c = (n - 1) / 2.0
    disk = (xx - c) ** 2 + (yy - c) ** 2 <= (DEMO_DISK * n) ** 2
    rng = np.random.default_rng(3)
    g = 40.0 + 150.0 * xx / (n - 1) + 50.0 * disk + rng.normal(0.0, 3.0, (n, n))
    img = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    u = 0.32 * n - np.sqrt((xx - c) ** 2 + (yy - c) ** 2)
    img.setflags(write=False)
    u.setflags(write=False)
    return [img], disk, u


@functools.lru_cache(maxsize=None)
def demo_reference():
    planes, _, u = demo_inputs()
    v = run(planes, u, DEMO_LOCAL, DEMO_RADIUS, DEMO_STEPS)[0]
    v.setflags(write=False)
    return v


# ---- the stop-rule case
STOP_CASE = (24, 64, 1, 4)


@functools.lru_cache(maxsize=None)
def stop_case():
    """(tol, k): with this tol the restatement stops at iteration k (1-based count of iterations done), 2 < k < 16, with a factor of
    at least 1.05 between the stop condition and the norms on either side of it"""
    h, w, C, rad = STOP_CASE
    planes, u = case_inputs(h, w, C)
    trace = run(planes, u, DEFAULT, rad, 15)[2]
    unit = R.stop_condition(planes, 1.0)
    worst = trace / unit   # the tol at which iteration t alone would pass
    for k in range(3, 15):
        before = worst[:k - 1].min()
        if worst[k - 1] * 1.05 ** 2 < before:
            tol = math.sqrt(worst[k - 1] * before)
            assert run(planes, u, dict(DEFAULT, tol=tol), rad, 40)[1] == k
            return tol, k
    raise AssertionError(f"no stopping iteration with a margin: {worst}")
