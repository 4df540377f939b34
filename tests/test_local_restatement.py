"""Local statistics without a GPU: the two restatements of the header's integer definition agree (local_util), the facts the header
states about the definition hold, the per-pixel arithmetic the kernels use (chan_vese_amd/csrc/local_math.h, compiled for the host and
exported by debug_exports.hip) gives the definition's values -- the floor square root for EVERY argument 0 .. 65025 --, and the
proposition itself on the CPU oracle: a disk that differs from its ground in texture alone is lost on the raw plane and found on the
local deviation plane."""
import ctypes
import math

import numpy as np
import pytest

import local_util as U


@pytest.fixture(scope="module")
def raw_lib():
    from chan_vese_amd import capi
    capi.lib()
    return ctypes.CDLL(capi.LIB_PATH)


@pytest.mark.parametrize("case", U.SMALL, ids=lambda c: "%dx%d-R%d" % c)
def test_the_two_restatements_agree(case):
    h, w, R = case
    for kind in ("random", "blocky", "all255"):
        plane = U.planes_of(kind, h, w, seed=R)[0]
        slow, quick = U.brute(plane, R), U.fast(plane, R)
        assert np.array_equal(slow[0], quick[0]) and np.array_equal(slow[1], quick[1]), kind


def test_constant_plane_and_radius_zero():
    for v in (0, 1, 128, 255):
        mean, dev = U.fast(np.full((9, 14), v, np.uint8), 3)
        assert (mean == v).all() and (dev == 0).all()
    plane = U.random_planes(12, 17)[0]
    mean, dev = U.fast(plane, 0)
    assert np.array_equal(mean, plane) and (dev == 0).all()
    mean, dev = U.brute(plane, 0)
    assert np.array_equal(mean, plane) and (dev == 0).all()


def test_half_and_half_window_gives_the_difference():
    for a, b in ((0, 255), (255, 0), (10, 13), (100, 101), (7, 7), (0, 1)):
        plane = np.empty((8, 8), np.uint8)          # columns 0 .. 3 are a, 4 .. 7 are b
        plane[:, :4], plane[:, 4:] = a, b
        for stats in (U.brute, U.fast):
            mean, dev = stats(plane, 127)           # every window is the whole plane: half a, half b
            assert (dev == abs(a - b)).all()
            assert (mean == (a + b + 1) // 2).all()  # round-half-up


def test_largest_sums():
    mean, dev = U.fast(np.full((256, 256), 255, np.uint8), 127)
    assert (mean == 255).all() and (dev == 0).all()
    n, S, Q = U.window_sums(np.full((300, 300), 255, np.uint8), 127)
    assert n.max() == 255 * 255 and S.max() == 255 ** 3 and Q.max() == 255 ** 4 < 2 ** 32
    assert 4 * int(n.max()) * int(Q.max()) < 2 ** 51


def test_results_stay_in_a_byte():
    for h, w, R, kind in [(40, 50, 1, "random"), (40, 50, 4, "blocky"), (64, 64, 20, "random"), (30, 90, 127, "blocky")]:
        plane = U.planes_of(kind, h, w)[0]
        n, S, Q = U.window_sums(plane, R)
        mean, q = (2 * S + n) // (2 * n), 4 * (n * Q - S * S) // (n * n)
        assert 0 <= mean.min() and mean.max() <= 255
        assert 0 <= q.min() and q.max() <= 255 * 255
    extreme = np.zeros((10, 10), np.uint8)          # the widest deviation there is: half 0, half 255
    extreme[:, 5:] = 255
    assert U.fast(extreme, 127)[1].max() == 255


def test_expected_planes_follow_the_pairing_rule():
    src3, src1 = U.random_planes(9, 11, 3), U.random_planes(9, 11, 1)
    got = U.expected(src1, 3, 2, U.STACK)
    assert np.array_equal(got[0], src1[0]) and np.array_equal(got[1], U.fast(src1[0], 2)[0]) and np.array_equal(got[2], U.fast(src1[0], 2)[1])
    got = U.expected(src3, 3, 1, (U.MEAN, U.COPY, U.DEV))
    assert np.array_equal(got[0], U.fast(src3[0], 1)[0]) and np.array_equal(got[1], src3[1]) and np.array_equal(got[2], U.fast(src3[2], 1)[1])
    assert np.array_equal(U.expected(src3, 1, 1, (U.MEAN, 9, 9))[0], U.fast(src3[0], 1)[0])     # entries behind C_dst are ignored
    assert all(np.array_equal(a, b) for a, b in zip(U.expected(src3, 3, 3, U.STACK, stats=U.brute), U.expected(src3, 3, 3, U.STACK)))


def test_isqrt_helper_is_the_floor_root_for_every_argument(raw_lib):
    """local_math.h's cvh_local_isqrt -- a float square root and an integer correction -- compiled for the host"""
    fn = raw_lib.cvh_debug_local_isqrt
    fn.restype, fn.argtypes = ctypes.c_uint, [ctypes.c_uint]
    for q in range(255 * 255 + 1):
        assert fn(q) == math.isqrt(q), q


def test_per_pixel_arithmetic_of_the_kernels_is_the_definition(raw_lib):
    """local_math.h's MEAN and DEV (an unsigned division; a double quotient with an integer correction) against Python integers:
    windows of real planes at every radius class, and the extremes of n, S and Q"""
    fn = raw_lib.cvh_debug_local_stats
    fn.restype, fn.argtypes = None, [ctypes.c_uint] * 3 + [ctypes.POINTER(ctypes.c_uint)] * 2
    rows = set()
    for h, w, R, kind in [(20, 23, 1, "random"), (20, 23, 3, "blocky"), (40, 41, 9, "blocky"), (64, 70, 127, "random")]:
        n, S, Q = U.window_sums(U.planes_of(kind, h, w, seed=3)[0], R)
        rows |= set(zip(n.ravel().tolist(), S.ravel().tolist(), Q.ravel().tolist()))
    big = 255 * 255
    for n in (1, 2, 3, 9, 25, 255, 4096, big - 1, big):                     # k pixels of value 255 or a, the others 0 or b
        for k in sorted({0, 1, n // 3, n // 2, (n + 1) // 2, n - 1, n}):
            for a, b in ((255, 0), (255, 254), (1, 0), (128, 127), (200, 13)):
                rows.add((n, k * a + (n - k) * b, k * a * a + (n - k) * b * b))
    mean, dev = ctypes.c_uint(), ctypes.c_uint()
    assert len(rows) > 2000
    for n, S, Q in rows:
        fn(n, S, Q, ctypes.byref(mean), ctypes.byref(dev))
        assert mean.value == (2 * S + n) // (2 * n), (n, S, Q)
        assert dev.value == math.isqrt(4 * (n * Q - S * S) // (n * n)), (n, S, Q)


def test_the_proposition_on_the_cpu_oracle():
    """128 x 128, 128 + noise: the sum of four uniform integers of -20 .. 20 inside the disk of radius 32 and of -5 .. 5 outside, from
    synth.splitmix64_stream(7, ..) (local_util.proposition_image) -- the same mean on both sides.  Checkerboard start, default
    parameters, 600 steps at most.  Measured on the oracle (steps, IoU with the disk, better of mask / inverted mask):
        raw plane                  1   0.166   (the run stops at once: there are no two means to separate)
        local deviation, R = 2   600   0.954   (the cap is reached)
    The bars are the issue's; the inputs are fixed integers and the oracle is deterministic."""
    raw, dev = U.oracle_proposition("raw"), U.oracle_proposition("dev")
    print("raw", raw[1], round(raw[2], 3), "dev", dev[1], round(dev[2], 3))
    assert raw[2] <= 0.3
    assert dev[2] >= 0.9
