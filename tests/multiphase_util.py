"""The four-phase (Vese-Chan) iteration of include/chanvese_hip.h, "Four phases", restated in numpy on np_restatement's heaviside /
delta / curvature -- what the device is compared against (test_gpu_multiphase.py) and what the CPU tests state facts about
(test_multiphase_restatement.py) -- with the test images, starts, parameter sets and cases.

Two forms of every sum: numpy's pairwise sum, and math.fsum over the flattened products (exactly rounded).  Their distance after a
case's iterations is the case's conditioning, which the GPU tolerance rests on."""
import functools
import math

import numpy as np

import np_restatement as R

LEVELS = (40, 100, 160, 220)   # background, disk 1 only, disk 2 only, both
DEFAULT = dict(mu=0.5, nu=0.0, dt=1.0, eps=1.0, tol=0.0, lambda1=(1.0, 1.0, 1.0), lambda2=(1.0, 1.0, 1.0))
# one non-default set, different mu, nu, dt and lambda in A and in B (eps must be equal)
OTHER_A = dict(mu=0.3, nu=0.05, dt=0.7, eps=1.0, tol=0.0, lambda1=(1.2, 0.9, 1.1), lambda2=(0.8, 1.1, 1.0))
OTHER_B = dict(mu=0.8, nu=-0.04, dt=0.9, eps=1.0, tol=0.0, lambda1=(0.7, 1.3, 1.0), lambda2=(1.1, 0.6, 1.2))
ITERATIONS = 6


def pairwise(a):
    return float(np.sum(a))


def exact(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


def disks_image(h, w, channels=1, noise=4.0, seed=11):
    """two overlapping disks, grey levels LEVELS on their four regions (channel k: the levels rotated by k), Gaussian noise"""
    yy, xx = np.mgrid[0:h, 0:w]
    s = max(h, w)
    cy = (h - 1) / 2.0
    d1 = (xx - (w - 1) * 0.36) ** 2 + (yy - cy) ** 2 <= (0.30 * s) ** 2
    d2 = (xx - (w - 1) * 0.64) ** 2 + (yy - cy) ** 2 <= (0.30 * s) ** 2
    cls = d1.astype(int) + 2 * d2.astype(int)
    rng = np.random.default_rng(seed)
    planes = []
    for k in range(channels):
        lev = np.array(LEVELS[k:] + LEVELS[:k], dtype=np.float64)
        g = lev[cls] + rng.normal(0.0, noise, (h, w))
        planes.append(np.clip(np.rint(g), 0, 255).astype(np.uint8))
    return planes, cls


def starts(h, w):
    """the reference's checkerboard and the same rolled by (2, 3) pixels (two identical starts stay identical forever)"""
    cb = R.checkerboard(h, w) + 0.0   # (no -0.0)
    return cb, np.roll(cb, (2, 3), axis=(0, 1))


def means(planes, u1, u2, eps=1.0, total=pairwise):
    """c[ab][k], ab in the order 11, 10, 01, 00"""
    h1, h2 = R.heaviside(u1, eps), R.heaviside(u2, eps)
    out = np.zeros((4, len(planes)))
    for ab, wt in enumerate((h1 * h2, h1 * (1 - h2), (1 - h1) * h2, (1 - h1) * (1 - h2))):
        den = total(wt)
        for k, img in enumerate(planes):
            out[ab, k] = total(img.astype(np.float64) * wt) / den
    return out


def step(planes, u1, u2, pa, pb, total=pairwise):
    """one Jacobi iteration: (new u1, new u2, the means it used, ||d1||, ||d2||)"""
    C = len(planes)
    eps = pa["eps"]
    c = means(planes, u1, u2, eps, total)
    h1, h2 = R.heaviside(u1, eps), R.heaviside(u2, eps)
    F1, F2 = np.zeros_like(u1), np.zeros_like(u2)
    for k, img in enumerate(planes):
        f = img.astype(np.float64)
        q11, q10, q01, q00 = ((f - c[ab, k]) ** 2 for ab in range(4))
        l1, l2 = pa["lambda1"][k], pa["lambda2"][k]
        F1 += h2 * (-l1 * q11 + l2 * q01) + (1 - h2) * (-l1 * q10 + l2 * q00)
        l1, l2 = pb["lambda1"][k], pb["lambda2"][k]
        F2 += h1 * (-l1 * q11 + l2 * q10) + (1 - h1) * (-l1 * q01 + l2 * q00)
    d1 = R.combine_folded(R.curvature(u1), F1, pa["mu"], pa["nu"], pa["dt"], C) * R.delta(u1, eps)
    d2 = R.combine_folded(R.curvature(u2), F2, pb["mu"], pb["nu"], pb["dt"], C) * R.delta(u2, eps)
    return u1 + d1, u2 + d2, c, math.sqrt(total(d1 * d1)), math.sqrt(total(d2 * d2))


def run(planes, u1, u2, pa, pb, max_steps, total=pairwise, stops=None):
    """cvh_multiphase_run: (u1, u2, steps_done, trace) -- a trace row is [c11[..], c10[..], c01[..], c00[..], ||d1||, ||d2||]"""
    if stops is None:
        stops = (R.stop_condition(planes, pa["tol"]), R.stop_condition(planes, pb["tol"]))
    rows = []
    for _ in range(max_steps):
        u1, u2, c, n1, n2 = step(planes, u1, u2, pa, pb, total)
        rows.append(list(c.ravel()) + [n1, n2])
        if n1 <= stops[0] and n2 <= stops[1]:
            break
    return u1, u2, len(rows), np.array(rows).reshape(len(rows), 4 * len(planes) + 2)


def labels(u1, u2):
    """mask as cvh_get_mask(invert = 0): (float)u > 0"""
    return ((u1.astype(np.float32) > 0).astype(np.uint8) + 2 * (u2.astype(np.float32) > 0).astype(np.uint8)).astype(np.uint8)


def near_zero(u1, u2, bound=1e-6):
    return (np.abs(u1) < bound) | (np.abs(u2) < bound)


def strip_rows(h, w):
    """rows per strip of the library's partition of an h x w plane (cvh_mp_geometry, multiphase_kernels.hip: about 4096 waves of 61
    columns, strips of a multiple of four rows, at least 8) -- restated here so that the cases exist without the library;
    test_multiphase_api.py holds the library to it for every case"""
    strips = max(4096 // -(-w // 61), 1)
    return max((-(-h // strips) + 3) & ~3, 8)


SEAM_H = strip_rows(1, 130) + 1   # one row past the strip length a short plane of 130 columns gets: two strips, the second of one row
assert strip_rows(SEAM_H, 130) == SEAM_H - 1


# (h, w, channels, parameter sets): the issue's shapes, then the ones this kernel's own geometry asks for -- 61 output columns per wave
# (lanes 2 .. 62): exactly one wave column, one lane past it, two full ones; a strip seam (one row past the 8-row strip at 130
# columns: the length is read from the code, cvh_mp_geometry, through cvh_multiphase_geometry)
# The checkerboard of a single row or column is identically zero (sin 0 = 0) and, with nu = 0 and equal lambdas, stays zero; that of
# 2 x 2 has one non-zero pixel.  Those three planes run the non-default sets, whose nu moves every pixel off zero.
CASES = [
    (1, 7, 1, "other"), (7, 1, 1, "other"), (2, 2, 1, "other"),
    (3, 130, 1, "default"), (67, 65, 3, "default"), (67, 65, 3, "other"), (24, 64, 1, "default"), (8, 4096, 1, "default"),
    (SEAM_H, 130, 1, "default"), (SEAM_H, 130, 1, "other"),
    (5, 61, 1, "default"), (6, 62, 1, "default"), (9, 122, 1, "other"),
]


def case_id(case):
    h, w, C, which = case
    return f"{h}x{w}x{C}-{which}"


def params_of(which):
    return (DEFAULT, DEFAULT) if which == "default" else (OTHER_A, OTHER_B)


@functools.lru_cache(maxsize=None)
def case_inputs(h, w, C):
    planes, _ = disks_image(h, w, C)
    u1, u2 = starts(h, w)
    for a in planes + [u1, u2]:
        a.setflags(write=False)
    return planes, u1, u2


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """the restatement's run of a case (pairwise sums): computed once, shared, read-only"""
    h, w, C, which = case
    planes, u1, u2 = case_inputs(h, w, C)
    pa, pb = params_of(which)
    v1, v2, steps, trace = run(planes, u1, u2, pa, pb, ITERATIONS)
    for a in (v1, v2, trace):
        a.setflags(write=False)
    return v1, v2, steps, trace


# ---- the stop-rule case: 24 x 64, default parameters but tol
STOP_SHAPE = (24, 64, 1)


@functools.lru_cache(maxsize=None)
def stop_case():
    """(tol, k): with this tol in both contexts the restatement stops at iteration k (1-based count of iterations done), 2 < k < 16,
    with a factor of at least 1.05 between the stop condition and the norms on either side of it"""
    planes, u1, u2 = case_inputs(*STOP_SHAPE)
    _, _, _, trace = run(planes, u1, u2, DEFAULT, DEFAULT, 15)
    unit = R.stop_condition(planes, 1.0)
    worst = np.maximum(trace[:, -2], trace[:, -1]) / unit   # the tol at which iteration t alone would pass
    for k in range(3, 15):
        before = worst[:k - 1].min()
        if worst[k - 1] * 1.05 ** 2 < before:
            tol = math.sqrt(worst[k - 1] * before)
            pa = dict(DEFAULT, tol=tol)
            assert run(planes, u1, u2, pa, pa, 40)[2] == k
            return tol, k
    raise AssertionError(f"no stopping iteration with a margin: {worst}")
