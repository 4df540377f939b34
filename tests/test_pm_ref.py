"""The reference of tests/test_gpu_pm_state.py, checked where no GPU is needed: pm_ref's restatement of a Perona-Malik step is the oracle
bit for bit in float64 on every case the GPU tests use, long double carries at least 63 mantissa bits, the oracle's own distance D_ref
from the long-double state is rounding noise (1e-14 .. 1e-12: the bar of the FAST planes is 8 x that, five orders of magnitude
below what the uint8 planes can show), and the tie planes put the oracle's state on k + 0.5 for even and odd k."""
import numpy as np
import pytest

import pm_ref


def oracle_state(oracle, img, klt):
    outs, states = oracle.perona_malik([img], *klt, want_state=True)
    return outs[0], states[0]


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("shape,klt", list(dict.fromkeys(pm_ref.CASES + pm_ref.ORIENTATION)))
def test_restatement_is_the_oracle_bit_for_bit_and_d_ref(oracle, shape, klt):
    img, trips, I_ld = pm_ref.reference(shape, klt)
    assert trips == oracle.pm_trip_count(klt[1], klt[2])
    out, state = oracle_state(oracle, img, klt)
    mine = pm_ref.perona_malik(img, klt[0], klt[1], trips, np.float64)
    assert mine.dtype == np.float64 and np.array_equal(mine.view(np.uint64), state.view(np.uint64))
    assert np.array_equal(pm_ref.to_u8(state), out)
    d_ref = float(np.abs(state.astype(np.longdouble) - I_ld).max())
    print(f"D_ref {shape[0]}x{shape[1]} K={klt[0]} trips={trips}: {d_ref:.2e}")
    # rounding noise of <= 80 steps on values <= 255 (ulp 2.8e-14): far below the 1.6e-6 a uint8 comparison can see, and not zero
    # wherever g is not identically 1 (a zero would mean the "long double" reference ran in double)
    assert d_ref <= 5e-12
    if min(shape) >= 3:
        assert d_ref > 0


def test_three_channel_planes_differ(oracle):
    a, b = pm_ref.rand_plane(18, 130, 0), pm_ref.rand_plane(18, 130, 2)
    assert not np.array_equal(a, b)
    img, trips, _ = pm_ref.reference((18, 130), pm_ref.P10, 2)
    _, state = oracle_state(oracle, img, pm_ref.P10)
    assert np.array_equal(pm_ref.perona_malik(img, 10, 0.25, trips).view(np.uint64), state.view(np.uint64))


def tie_planes():
    line = pm_ref.TIE_LINE
    return {"1xN": (line[None, :].copy(), pm_ref.TIE_K), "Nx1": (line[:, None].copy(), pm_ref.TIE_K),
            "16xN flat g": (np.tile(line, (16, 1)), pm_ref.TIE_K_FLAT), "Nx16 flat g": (np.tile(line[:, None], (1, 16)), pm_ref.TIE_K_FLAT)}


@pytest.mark.parametrize("name", list(tie_planes()))
def test_tie_planes_put_the_oracle_on_exact_ties_of_both_parities(oracle, name):
    img, K = tie_planes()[name]
    out, state = oracle_state(oracle, img, (K, pm_ref.TIE_L, pm_ref.TIE_T))
    assert oracle.pm_trip_count(pm_ref.TIE_L, pm_ref.TIE_T) == 1
    even, odd = pm_ref.count_ties(state)
    assert even >= 8 and odd >= 8, (even, odd)
    # the exact value: I0 + (sum of the four differences) / 8, and the rounding of every tie goes to the even neighbour
    i0 = img.astype(np.int64)
    p = np.pad(i0, 1, mode="edge")
    lap = p[2:, 1:-1] + p[:-2, 1:-1] + p[1:-1, 2:] + p[1:-1, :-2] - 4 * i0
    assert np.array_equal(state, i0 + lap / 8.0)
    tie = (state - np.floor(state)) == 0.5
    assert (out[tie] % 2 == 0).all()
    for dt in (np.float64, np.longdouble):
        assert np.array_equal(pm_ref.perona_malik(img, K, pm_ref.TIE_L, 1, dt), state)
