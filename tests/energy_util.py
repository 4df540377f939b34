"""numpy restatement of the Chan-Sandberg-Vese functional as include/chanvese_hip.h defines it ("Energy"), and the inputs the energy tests
share.  Every term is a sum of per-pixel products taken with math.fsum -- exactly rounded --, so a comparison against it measures the
code under test alone.  Shared by test_energy_api.py (CPU, on the oracle) and test_gpu_energy.py."""
import functools
import math

import numpy as np

from pyramid_util import SHAPES, CHANNELS, planes_of, smooth_levelset   # noqa: F401  (the energy tests use the pyramid's shapes and inputs)

SAMPLES = [0] + [1 << k for k in range(10)]   # iterations at which the proposition samples the energy: 0, 1, 2, 4, ..., 512


def _sum(a):
    """the exactly rounded sum of a's finite entries; IEEE's answer where an entry is not finite"""
    a = np.asarray(a, dtype=np.float64).ravel()
    if not np.isfinite(a).all():
        with np.errstate(invalid="ignore"):
            return float(np.sum(a))
    return math.fsum(a.tolist())


def heaviside(u, eps):
    return 0.5 * (1.0 + (2.0 / math.pi) * np.arctan(u / eps))


def delta(u, eps):
    return eps / (math.pi * (eps * eps + u * u))


def means(planes, u, eps=1.0):
    """c1 / c2 of the definition: sum I H / sum H and sum I (1 - H) / sum (1 - H), exact sums"""
    hv = heaviside(np.asarray(u, dtype=np.float64), eps)
    c1 = [_sum(p.astype(np.float64) * hv) / _sum(hv) for p in planes]
    c2 = [_sum(p.astype(np.float64) * (1.0 - hv)) / _sum(1.0 - hv) for p in planes]
    return np.array(c1), np.array(c2)


def terms(planes, u, mu=0.5, nu=0.0, eps=1.0, lambda1=None, lambda2=None, c1=None, c2=None):
    """dict(total, length, area, fit_in[C], fit_out[C], c1[C], c2[C]) of the level set u over the uint8 planes.  c1 / c2: the means to
    take the fit terms with (what cvh_get_means returned); None: this module's own."""
    u = np.asarray(u, dtype=np.float64)
    h, w = u.shape
    C = len(planes)
    lambda1 = [1.0] * C if lambda1 is None else list(lambda1)
    lambda2 = [1.0] * C if lambda2 is None else list(lambda2)
    if c1 is None or c2 is None:
        c1, c2 = means(planes, u, eps)
    with np.errstate(invalid="ignore", over="ignore"):
        cols, rows = np.arange(w), np.arange(h)
        gx = (u[:, np.minimum(cols + 1, w - 1)] - u[:, np.maximum(cols - 1, 0)]) * 0.5
        gy = (u[np.minimum(rows + 1, h - 1), :] - u[np.maximum(rows - 1, 0), :]) * 0.5
        hv = heaviside(u, eps)
        length = _sum(delta(u, eps) * np.sqrt(gx * gx + gy * gy))
        area = _sum(hv)
        fit_in = [_sum((p.astype(np.float64) - c1[k]) ** 2 * hv) for k, p in enumerate(planes)]
        fit_out = [_sum((p.astype(np.float64) - c2[k]) ** 2 * (1.0 - hv)) for k, p in enumerate(planes)]
        fit = None
        for k in range(C):
            t = lambda1[k] * fit_in[k] + lambda2[k] * fit_out[k]
            fit = t if fit is None else fit + t
        total = mu * length + nu * area + (1.0 / C) * fit
    return dict(total=total, length=length, area=area, fit_in=fit_in, fit_out=fit_out, c1=list(c1), c2=list(c2))


def flat(t):
    """the term values of terms()' dict or of a capi.Energy in one order: total, length, area, fit_in.., fit_out.."""
    get = t.get if isinstance(t, dict) else (lambda k: getattr(t, k))
    return np.array([get("total"), get("length"), get("area"), *get("fit_in"), *get("fit_out")], dtype=np.float64)


def planted_levelset(h, w):
    """smooth_levelset with +inf, -inf and NaN planted: a corner, the last column, the interior"""
    u = smooth_levelset(h, w).copy()
    u[0, 0] = np.inf
    u[h // 2, w - 1] = -np.inf
    u[h // 3, w // 3] = np.nan
    return u


def inf_levelset(h, w):
    """smooth_levelset with one +inf and one -inf planted and no NaN: the terms the infinities do not reach stay finite"""
    u = smooth_levelset(h, w).copy()
    u[h - 1, 0] = np.inf
    u[h // 2, w // 2] = -np.inf
    return u


@functools.lru_cache(maxsize=None)
def oracle_series(n, sign=1):
    """The issue's proposition on the CPU oracle: synth.disk(n, noise=32, seed=3), the (signed) checkerboard start, default parameters,
    tol = 0.  Returns (img, [(iterations, terms)] at SAMPLES).  Computed once per process; callers must not modify it."""
    from chan_vese_amd import synth
    from oracle import cv_oracle as O
    img = synth.disk(n, noise=32, seed=3)
    p = O.make_params(tol=0.0)
    u = sign * O.checkerboard(n, n)
    out, at = [(0, terms([img], u))], 0
    for s in SAMPLES[1:]:
        u, done, _, _ = O.csv_run([img], u, p, s - at, trace=False)
        assert done == s - at
        at = s
        out.append((s, terms([img], u)))
    return img, out
