"""The fixture of tests/test_gpu_csv_math.py (tests/golden/csv_math_ref.npz): it equals a fresh high-precision computation, and its
arguments reach every form the FAST per-pixel arithmetic takes -- every cell j in [-128, 128] of the near table and both sides of each
cell boundary, of a = 1, of the far threshold 32 eps and of the 1e300 clamp, for every eps."""
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "csv_math_ref.npz")))


def _generator():
    spec = importlib.util.spec_from_file_location("make_csv_math_ref", os.path.join(GOLDEN, "make_csv_math_ref.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.skipif(importlib.util.find_spec("mpmath") is None, reason="the generator needs mpmath")
def test_fixture_equals_a_fresh_computation(ref):
    fresh = _generator().compute()
    assert sorted(fresh) == sorted(ref)
    for k, v in fresh.items():
        assert v.dtype == ref[k].dtype and v.shape == ref[k].shape, k
        assert v.tobytes() == ref[k].tobytes(), k    # bit for bit, signed zeros included


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(GOLDEN, "csv_math_ref.npz")) < 256 << 10


def test_h_arguments_cover_every_table_cell_and_both_sides_of_every_edge(ref):
    x, eps_i = ref["h_x"], ref["h_eps"]
    for ie, eps in enumerate(ref["eps"]):
        xe = x[eps_i == ie]
        a = np.abs(xe) / eps
        fin = np.isfinite(a)
        j = np.rint(np.where(fin, (a - 1) / np.where(fin, a + 1, 1.0), 1.0) * 128).astype(int)
        assert set(j) == set(range(-128, 129)), (eps, sorted(set(range(-128, 129)) - set(j)))
        # both sides of every cell boundary (a - 1)/(a + 1) = (j + 1/2)/128, in exact arithmetic, within 1e-12
        E = Fraction(float(eps))
        near = [Fraction(float(v)) / E for v in np.abs(xe) if 0 < v < 1e6 * eps]
        ys = sorted((A - 1) / (A + 1) for A in near)
        ys_f = np.array([float(y) for y in ys])
        for jb in range(-128, 128):
            b = Fraction(2 * jb + 1, 256)
            lo = np.searchsorted(ys_f, float(b) - 1e-12)
            hi = np.searchsorted(ys_f, float(b) + 1e-12)
            window = ys[lo:hi]
            assert any(y < b for y in window) and any(y > b for y in window), (eps, jb)
        thr = 32.0 * eps
        for edge, name in ((thr, "far threshold"), (eps, "a = 1"), (1e300 * eps, "1e300 clamp")):
            below = xe[(np.abs(xe) < edge) & (np.abs(xe) >= np.nextafter(edge, 0) - 4 * np.spacing(edge))]
            above = xe[(np.abs(xe) > edge) & (np.abs(xe) <= edge + 4 * np.spacing(edge))]
            assert len(below) and len(above) and np.any(np.abs(xe) == edge), (eps, name)
        assert len(set(np.abs(xe[(np.abs(xe) < thr) & (np.abs(xe) >= thr - 8 * np.spacing(thr))]))) >= 4, eps   # 1..4 ulp below
        assert len(set(np.abs(xe[(np.abs(xe) > thr) & (np.abs(xe) <= thr + 8 * np.spacing(thr))]))) >= 4, eps   # 1..4 ulp above
        # the band where a 16-eps threshold would already use the far series, the range where a +- 1 rounds, subnormals, signed zeros
        assert np.sum((np.abs(xe) >= 16 * eps) & (np.abs(xe) < thr)) >= 10, eps
        assert np.sum((a >= 1e6) & (a <= 1e17)) >= 20, eps
        assert np.any((xe != 0) & (np.abs(xe) < 2.2250738585072014e-308))
        z = xe[xe == 0]
        assert np.any(np.signbit(z)) and np.any(~np.signbit(z))
        assert np.min(np.abs(xe[xe != 0])) <= 1e-300 and np.max(np.abs(xe)) >= 1e300 * eps


def test_references_are_consistent(ref):
    """Cheap double-precision cross-checks of the stored references (each within a few ulp of numpy's own evaluation)."""
    x, eps = ref["h_x"], ref["eps"][ref["h_eps"]]
    np_h = np.arctan(np.abs(x) / eps) / np.pi * np.where(np.signbit(x), -1.0, 1.0)
    assert np.all(np.abs(ref["h_ref"] - np_h) <= 4 * np.spacing(0.5))
    assert np.array_equal(np.signbit(ref["h_ref"]), np.signbit(x))
    assert np.all(np.abs(ref["h_strict"] - (0.5 + np_h)) <= 4 * np.spacing(0.5))
    assert ref["h_far_clamp"] == pytest.approx(np.arctan(32.0) / np.pi, abs=1e-16)
    assert np.allclose(ref["rcp_hi"], 1 / ref["rcp_x"], rtol=2.3e-16, atol=0)
    assert np.allclose(ref["rsq_hi"], 1 / np.sqrt(ref["rsq_x"]), rtol=4.5e-16, atol=0)
    assert np.all(np.abs(ref["rcp_lo"]) <= 0.5 * np.spacing(np.abs(ref["rcp_hi"])))
    assert np.all(np.abs(ref["rsq_lo"]) <= 0.5 * np.spacing(np.abs(ref["rsq_hi"])))


def test_far_series_truncation_at_the_threshold():
    """The far form sums atan(t)/pi, t = eps/|u| <= 1/32, through t^9/9 (k0..k4 of wave_math.h).  The alternating series' remainder is
    below its first omitted term: t^11/(11 pi) < 8.1e-19 in H at the threshold -- under the 2.5e-18 the issue sets (in atan itself,
    t^11/11 = 2.52e-18).  Exact rational arithmetic."""
    t = Fraction(1, 32)
    first_omitted = t ** 11 / 11
    pi_lo = Fraction(314159265358979, 10 ** 14)
    assert first_omitted / pi_lo < Fraction(81, 10 ** 20)
    assert first_omitted / pi_lo < Fraction(25, 10 ** 19)
    # a threshold of 16 eps with the same 5 terms would truncate at t^11/(11 pi) = 1.6e-15 -- seven ulp of 1/2
    assert (Fraction(1, 16) ** 11 / 11) / pi_lo > 7 * Fraction(1, 2 ** 53)
