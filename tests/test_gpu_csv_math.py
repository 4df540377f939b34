"""The FAST flavour's per-pixel arithmetic on the device, function by function, against tests/golden/csv_math_ref.npz (mpmath at 50
digits, rounded once; tests/golden/make_csv_math_ref.py).  cvh_debug_csv_math runs the very inline functions of wave_math.h and
csv_device.h that the step kernels call, with the atan tables api.hip fills (the near table staged in LDS) and the far-field series
csv_run.hip sets up.  Through whole steps an error of H is averaged into c1 / c2 and hides below the 1e-9 bars of the parity tests;
here every form is held to its own claim at the arguments where it changes form (see the generator: table-cell boundaries, a = 1,
32 eps, the 1e300 clamp, subnormals, signed zeros, 1e-8 .. 1e300) for eps in {0.05, 0.5, 1, 2, 16}.  The bars are in ulp:
ULP_HALF = 2^-53 is one ulp of 1/2."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ULP_HALF = 2.0 ** -53
(H_FAR, H_NEAR, H_FAST, H_STRICT, ATAN_TABLE, INV_DELTA, DELTA, INV_DELTA_TILE, DELTA_TILE, RCP, RSQRT, NORMALISED,
 NORMALISED4) = range(13)


@pytest.fixture(scope="module")
def ref():
    return dict(np.load(os.path.join(GOLDEN, "csv_math_ref.npz")))


@pytest.fixture(scope="module")
def math():
    from chan_vese_amd import capi
    L = capi.lib()
    assert capi.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    fn = L.cvh_debug_csv_math
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_double)]
    arity = L.cvh_debug_csv_math_arity
    arity.restype, arity.argtypes = C.c_int, [C.c_int]

    def run(op, x, eps=1.0):
        x = np.ascontiguousarray(x, dtype=np.float64)
        n = x.shape[-1]
        assert x.size == arity(op) * n
        out = np.empty(n)
        rc = fn(op, n, x.ctypes.data_as(C.POINTER(C.c_double)), float(eps), out.ctypes.data_as(C.POINTER(C.c_double)))
        assert rc == 0, (rc, L.cvh_last_error(None))
        return out
    return run


def rel_ulp(got, hi, lo=None):
    """|got - exact| in ulp of the correctly rounded exact value (exact = hi + lo)."""
    d = (got - hi) - (lo if lo is not None else 0.0)
    return np.abs(d) / np.spacing(np.abs(hi))


def h_case(ref, ie):
    sel = ref["h_eps"] == ie
    return float(ref["eps"][ie]), ref["h_x"][sel], ref["h_ref"][sel], ref["h_strict"][sel]


@pytest.mark.parametrize("ie", range(5))
def test_heaviside_far_near_and_combined(math, ref, ie):
    """H_eps - 1/2 (the sums carry it centred) within 2 ulp of 1/2, absolute, at every finite argument, in each form:
    - near (heaviside_centred_near, any argument): atan(c) from a table rounded once (1/2 ulp), |z| <= 1/256 so the series z - z^3/3 +
      z^5/5 truncates below 2e-18, n = a - 1 and d = a + 1 rounded once each (<= 1/2 ulp of 1 in y, times atan' <= 1, divided by pi),
      the refined reciprocal (<= 1 ulp of z) and the last fma (1/2 ulp): 2 ulp of 1/2 holds with room;
    - far (heaviside_centred_far) from 32 eps on: the series truncation t^11/(11 pi) < 8.1e-19 (tests/test_csv_math_ref.py), the
      refined reciprocal and the fused fold: the same bar; below 32 eps the argument is CLAMPED to 32 eps, so there the bar is
      against atan(32)/pi with the argument's sign;
    - combined (far + near_field_correction: what the wave / resident kernels' sums carry): the near form within one more rounding.
    The sign follows the argument, +-0 included (the combined form: see below)."""
    eps, x, h, _ = h_case(ref, ie)
    thr = 32.0 * eps
    far_ref = np.where(np.abs(x) >= thr, h, np.copysign(ref["h_far_clamp"], x))
    bars = {}
    for op, name, want in ((H_NEAR, "near", h), (H_FAR, "far", far_ref), (H_FAST, "combined", h)):
        got = math(op, x, eps)
        assert np.all(np.isfinite(got)), name
        err = np.abs(got - want)
        bars[name] = err.max() / ULP_HALF
        worst = int(np.argmax(err))
        assert err.max() <= 2 * ULP_HALF, (name, eps, x[worst], got[worst], want[worst], err.max() / ULP_HALF)
        # the sign follows the argument -- in the combined form only where |H - 1/2| exceeds the bar: at +-0 and at arguments below
        # ~2e-16 eps, far (-atan(32)/pi) + correction (+atan(32)/pi) cancels to +0 exactly, an absolute error below 1e-16 eps that
        # no sum can tell from the exact value (measured: -0, -5e-324, -1e-300 give +0)
        signed = np.abs(want) > 2 * ULP_HALF if op == H_FAST else np.ones(x.shape, bool)
        assert np.array_equal(np.signbit(got[signed]), np.signbit(x[signed])), (name, eps, x[signed & (np.signbit(got) != np.signbit(x))][:5])
    print(f"eps {eps}: max |err| / ulp(1/2): " + ", ".join(f"{k} {v:.3f}" for k, v in bars.items()))


@pytest.mark.parametrize("ie", range(5))
def test_heaviside_strict(math, ref, ie):
    """STRICT H_eps (1 + 2/pi atan(x/eps)) / 2 with the device's libm atan and IEEE division: within 4 ulp of 1/2, absolute -- x / eps
    rounded (1/2 ulp, times x atan'(x) <= 1/2, over pi), ocml's atan (<= 2 ulp of pi/2 at most, times 2/pi), 2/pi and the product
    rounded, 1 + t rounded to 1/2 ulp of 1 and halved: about 2.6 ulp of 1/2 in the worst case."""
    eps, x, _, hs = h_case(ref, ie)
    got = math(H_STRICT, x, eps)
    err = np.abs(got - hs)
    worst = int(np.argmax(err))
    assert err.max() <= 4 * ULP_HALF, (eps, x[worst], got[worst], hs[worst], err.max() / ULP_HALF)
    print(f"eps {eps}: strict max |err| / ulp(1/2) {err.max() / ULP_HALF:.3f}")


def test_atan_table(math, ref):
    """atan_table (the tile kernel's FAST atan, used as H = 1/2 + atan/pi): table value rounded once, one Newton-refined reciprocal,
    one final addition -- within 2 ulp of atan(x), relative -- plus the series z - z^3/3 + z^5/5 truncated at |z| <= 1/256: up to
    (1/256)^7/7 = 1.98e-18 ABSOLUTE.  In cell 0 (atan(x) ~ x < 1/256) that is 5 ulp relative (measured: 5.0 ulp at x = 1/256 - 1 ulp),
    1/50 of an ulp of the H it feeds.  On both branches (|x| <= 1 and 1/|x|), every cell boundary, the switch at 1, the 1e300 clamp;
    exact +-0 at +-0."""
    x, want = ref["at_x"], ref["at_ref"]
    got = math(ATAN_TABLE, x)
    e = np.abs(got - want) / (2 * np.spacing(np.abs(want)) + 2.0 ** -58)      # 2 ulp + the truncation bound, rounded up to 2^-58
    worst = int(np.argmax(e))
    assert e.max() <= 1.0, (x[worst], got[worst], want[worst], rel_ulp(got, want)[worst])
    assert np.array_equal(np.signbit(got), np.signbit(x))
    print(f"atan_table max err {rel_ulp(got, want).max():.3f} ulp, {np.abs(got - want).max():.3e} absolute")


@pytest.mark.parametrize("ie", range(5))
def test_delta_forms(math, ref, ie):
    """1/delta_eps(u) = (pi/eps)(eps^2 + u^2) as the wave / resident kernels form it (fma(u, u, eps^2) * pi/eps: eps^2, pi/eps, the fma
    and the product rounded once each) and as the tile kernel does (fma(u^2, pi/eps, pi eps)): within 3 ulp, relative; delta_eps =
    rcp_refined of it: one more ulp (4).  Over |u| <= 1e150, where u^2 is finite."""
    sel = ref["d_eps"] == ie
    eps, x, inv, dl = float(ref["eps"][ie]), ref["d_x"][sel], ref["d_inv"][sel], ref["d_ref"][sel]
    for op_inv, op_d, name in ((INV_DELTA, DELTA, "wave"), (INV_DELTA_TILE, DELTA_TILE, "tile")):
        gi, gd = math(op_inv, x, eps), math(op_d, x, eps)
        ei, ed = rel_ulp(gi, inv), rel_ulp(gd, dl)
        assert ei.max() <= 3.0, (name, eps, x[int(np.argmax(ei))], ei.max())
        assert ed.max() <= 4.0, (name, eps, x[int(np.argmax(ed))], ed.max())
        print(f"eps {eps} {name}: 1/delta {ei.max():.3f} ulp, delta {ed.max():.3f} ulp")


@pytest.mark.parametrize("op,key", [(RCP, "rcp"), (RSQRT, "rsq")])
def test_refined_reciprocal_and_rsqrt(math, ref, op, key):
    """rcp_refined / rsqrt_refined: the code claims <= 1 ulp from the hardware estimate after one cubic step; held to 1 ulp of the
    exact value, relative, over the normal range (powers of two and their neighbours from 2^-1020 to 2^1020, random mantissas)."""
    x, hi, lo = ref[key + "_x"], ref[key + "_hi"], ref[key + "_lo"]
    got = math(op, x)
    e = rel_ulp(got, hi, lo)
    worst = int(np.argmax(e))
    assert e.max() <= 1.0, (key, x[worst], got[worst], hi[worst], e.max())
    print(f"{key} max err {e.max():.3f} ulp")


def test_normalised_forms(math, ref):
    """normalised<true>(d+, d0) and normalised4(fwd, bwd, 2c) -- d+ / sqrt(d+^2 + d0^2 + eta^2) -- with gradients at eta = 1e-8, ordinary
    and large ones (up to 1e150): squares and the sum rounded (the fma chain: <= 1.5 ulp of s), rsqrt_refined (1 ulp), sqrt halves the
    relative error of s, the last product (1/2 ulp): within 3 ulp of the exact value, relative; 0 exactly where d+ = 0."""
    for op, key in ((NORMALISED, "n2"), (NORMALISED4, "n4")):
        x, want = ref[key + "_x"], ref[key + "_ref"]
        got = math(op, x)
        e = np.where(want == 0, np.abs(got), rel_ulp(got, want))
        worst = int(np.argmax(e))
        assert e.max() <= 3.0, (key, x[:, worst], got[worst], want[worst], e.max())
        print(f"{key} max err {e.max():.3f} ulp")
