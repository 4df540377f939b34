"""Writes tests/golden/csv_math_ref.npz: arguments of the FAST flavour's per-pixel arithmetic (wave_math.h, csv_device.h) at the
edges where it changes form, with references computed by mpmath at 50 significant digits and rounded once to double.

    python tests/golden/make_csv_math_ref.py

tests/test_csv_math_ref.py recomputes the fixture (when mpmath is importable) and checks what the arguments cover;
tests/test_gpu_csv_math.py holds the device functions against it.  Arrays:

  h_x, h_eps (index into eps), h_ref     H_eps(x) - 1/2 = copysign(atan(|x|/eps)/pi, x) (+-0 at +-0)
  h_strict                               H_eps(x) = 1/2 + atan(x/eps)/pi
  h_far_clamp                            atan(32)/pi: the far form's value below its threshold 32 eps (any eps)
  at_x, at_ref                           atan(x)
  d_x, d_eps, d_inv, d_ref               1/delta_eps(x) = pi (eps^2 + x^2) / eps and delta_eps(x)
  rcp_x, rcp_hi, rcp_lo                  1/x as hi + lo (hi correctly rounded, lo the rounded remainder)
  rsq_x, rsq_hi, rsq_lo                  1/sqrt(x) the same way
  n2_x (2 x m), n2_ref                   up / sqrt(up^2 + uc^2 + eta^2), eta^2 = 1e-8 * 1e-8 as a double (kEta2)
  n4_x (3 x m), n4_ref                   d+ / sqrt(d+^2 + d0^2 + eta^2), d+ = fwd - c, d0 = (fwd - bwd) / 2: (fwd, bwd, 2c), differences exact
"""
import os

import numpy as np

EPS = (0.05, 0.5, 1.0, 2.0, 16.0)
DPS = 50
ETA2 = 1e-8 * 1e-8
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csv_math_ref.npz")


def _steps(x, k):
    """x moved by k ulp (k < 0: down)."""
    x = float(x)
    for _ in range(abs(k)):
        x = float(np.nextafter(x, np.inf if k > 0 else -np.inf))
    return x


def h_inputs(eps, mp):
    xs = [0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, 1e-300, -1e-300]
    # both sides of every near-table cell boundary: (a - 1)/(a + 1) * 128 = j + 1/2, a = |x| / eps
    for jb in range(-128, 128):
        y = mp.mpf(2 * jb + 1) / 256
        u0 = float((1 + y) / (1 - y) * eps)
        xs += [_steps(u0, k) for k in (-3, -1, 0, 1, 3)]
    for j in range(-127, 128):                                              # the middle of every cell (j = +-128: a -> 0, a -> inf)
        y = mp.mpf(j) / 128
        xs.append(float((1 + y) / (1 - y) * eps))
    xs += [_steps(eps, k) for k in (-2, -1, 0, 1, 2)]                       # a = 1 +- ulp
    xs += [_steps(32.0 * eps, k) for k in range(-4, 5)]                     # the far threshold +- 1..4 ulp
    xs += [-_steps(32.0 * eps, k) for k in (-1, 0, 1)]
    xs += list(np.geomspace(1e-8, 1e300, 500))                              # dense sweep
    xs += [-v for v in np.geomspace(1e-8, 1e300, 100)]
    xs += list(np.geomspace(1e-3 * eps, 64.0 * eps, 128))                   # the near field and the band below the threshold
    xs += [a * eps for a in np.geomspace(1e6, 1e17, 40)]                    # a +- 1 rounds
    xs += [_steps(1e300 * eps, k) for k in (-2, -1, 0, 1, 2)] + [1e301 * eps, -1e300 * eps, 1.7976931348623157e308]
    return np.array(xs, dtype=np.float64)


def compute():
    import mpmath as mp
    mp.mp.dps = DPS
    pi = mp.pi
    r = {"eps": np.array(EPS)}
    hx, he, href, hstr = [], [], [], []
    for ie, eps in enumerate(EPS):
        for x in h_inputs(eps, mp):
            a = mp.atan(mp.fabs(mp.mpf(x)) / eps) / pi
            hx.append(x); he.append(ie)
            href.append(float(a) if not np.signbit(x) else -float(a))
            hstr.append(float(mp.mpf(1) / 2 + mp.atan(mp.mpf(x) / eps) / pi))
    r.update(h_x=np.array(hx), h_eps=np.array(he, dtype=np.int8), h_ref=np.array(href), h_strict=np.array(hstr),
             h_far_clamp=np.array(float(mp.atan(32) / pi)))
    # atan_table: cell boundaries of c = i/128 on both branches, the switch at 1, the clamp at 1e300, a sweep
    ax = [0.0, -0.0, 1e-300, 1.0, -1.0, _steps(1.0, -1), _steps(1.0, 1), 1e300, _steps(1e300, 1), 1e308, -1e308]
    for i in range(128):
        b = (i + 0.5) / 128
        ax += [_steps(b, k) for k in (-1, 1)] + [_steps(1 / b, k) for k in (-1, 1)]
    ax += list(np.geomspace(1e-10, 1e20, 300)) + [-v for v in np.geomspace(1e-6, 1e6, 40)]
    r["at_x"] = np.array(ax)
    r["at_ref"] = np.array([float(mp.atan(mp.mpf(x))) for x in ax])
    # delta_eps: finite range of x^2 (|x| <= 1e150)
    dx, de, dinv, dref = [], [], [], []
    for ie, eps in enumerate(EPS):
        for x in [0.0, -0.0, 1e-300, _steps(eps, 1), eps, -eps, 32.0 * eps] + list(np.geomspace(1e-8, 1e150, 120)) + [-v for v in np.geomspace(1e-4, 1e4, 20)]:
            q = pi * (mp.mpf(eps) ** 2 + mp.mpf(x) ** 2) / eps
            dx.append(x); de.append(ie); dinv.append(float(q)); dref.append(float(1 / q))
    r.update(d_x=np.array(dx), d_eps=np.array(de, dtype=np.int8), d_inv=np.array(dinv), d_ref=np.array(dref))
    # refined reciprocal / rsqrt over the normal range: powers of two, their neighbours, mantissa patterns, a sweep
    rng = np.random.default_rng(7)
    base = [2.0 ** e for e in range(-1020, 1021, 17)]
    vals = base + [_steps(v, 1) for v in base] + [_steps(v, -1) for v in base]
    vals += list(rng.uniform(1, 2, 400) * 2.0 ** rng.integers(-1000, 1000, 400))
    vals += [1.0, 3.0, 1.5, _steps(2.0, -1), 1e-300, 1e300, 1e-16, 4e-16]
    for name, f in (("rcp", lambda v: 1 / v), ("rsq", lambda v: 1 / mp.sqrt(v))):
        xs = np.array(vals + ([-v for v in vals[:200]] if name == "rcp" else []))
        hi, lo = [], []
        for x in xs:
            e = f(mp.mpf(x))
            h = float(e)
            hi.append(h); lo.append(float(e - h))
        r[name + "_x"], r[name + "_hi"], r[name + "_lo"] = xs, np.array(hi), np.array(lo)
    # normalised<true>(up, uc): gradients near eta = 1e-8, ordinary and large ones (|up|, |uc| <= 1e150)
    ups, ucs = [], []
    mags = [0.0, 1e-12, 1e-9, 5e-9, 1e-8, 2e-8, 1e-7, 1e-3, 1.0, 37.0, 1e4, 1e8, 1e100, 1e150]
    for m1 in mags:
        for m2 in mags:
            for s1, s2 in ((1, 1), (-1, 1), (1, -1)):
                ups.append(s1 * m1); ucs.append(s2 * m2)
    ups += list(rng.normal(scale=1e-8, size=100)) + list(rng.normal(scale=10, size=100))
    ucs += list(rng.normal(scale=1e-8, size=100)) + list(rng.normal(scale=10, size=100))
    e2 = mp.mpf(ETA2)
    r["n2_x"] = np.array([ups, ucs])
    r["n2_ref"] = np.array([float(mp.mpf(u) / mp.sqrt(mp.mpf(u) ** 2 + mp.mpf(v) ** 2 + e2)) for u, v in zip(ups, ucs)])
    # normalised4(fwd, bwd, 2c): triples whose differences fwd - c and fwd - bwd are exact doubles (what the kernels' samples give)
    trip = []
    for c in [0.0, 1.0, -3.5, 100.0, 1e4]:
        for dp in [0.0, 1e-9, -1e-8, 3e-8, 0.25, -7.0, 1e3]:
            for dm in [0.0, 2e-9, -1e-8, 0.5, 12.0]:
                trip.append((c + dp, c - dm, c))
    for _ in range(300):
        c = rng.normal(scale=50)
        trip.append((c + rng.normal(scale=rng.choice([1e-8, 1.0, 100.0])), c + rng.normal(scale=rng.choice([1e-8, 1.0, 100.0])), c))
    keep = []
    for f, b, c in trip:
        F, B, Cc = mp.mpf(f), mp.mpf(b), mp.mpf(c)
        if mp.mpf(f - c) == F - Cc and mp.mpf(f - b) == F - B:
            keep.append((f, b, c))
    n4x = np.array([[f for f, _, _ in keep], [b for _, b, _ in keep], [2.0 * c for _, _, c in keep]])
    ref = []
    for f, b, c in keep:
        dp, d0 = mp.mpf(f) - mp.mpf(c), (mp.mpf(f) - mp.mpf(b)) / 2
        ref.append(float(dp / mp.sqrt(dp * dp + d0 * d0 + e2)))
    r["n4_x"], r["n4_ref"] = n4x, np.array(ref)
    return r


if __name__ == "__main__":
    r = compute()
    np.savez_compressed(OUT, **r)
    print(OUT, os.path.getsize(OUT), "bytes;", ", ".join(f"{k} {v.shape}" for k, v in r.items()))
