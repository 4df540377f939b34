"""Rank planes without a GPU: the two restatements of the header's definition agree (rank_util), the facts the header states about the
definition hold, the integer arithmetic the kernels share with the host (chan_vese_amd/csrc/rank_math.h, compiled for the host and
exported by debug_exports.hip) gives the definition's values, and the two propositions themselves on the CPU oracle: a disk under salt
and pepper is lost on the raw plane and found on the median plane; blobs on a shading ramp are lost on the raw plane and found on the
white top-hat."""
import ctypes

import numpy as np
import pytest

import rank_util as U


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
        for code in U.CODES:
            r = min(R, U.MEDIAN_RADIUS_MAX) if code == U.MEDIAN else R
            assert np.array_equal(U.brute(plane, r, code), U.fast(plane, r, code)), (kind, code)


def test_scipy_and_the_running_extrema_agree_on_the_truncated_window():
    plane = U.blocky_planes(40, 53, seed=2)[0]
    for R in (16, 20, 127):
        for op in (np.minimum, np.maximum):
            assert np.array_equal(U._extreme(plane, R, op), U._running(U._running(plane, R, 1, op), R, 0, op))


@pytest.mark.parametrize("R", [1, 2, 5, 9])
def test_properties_of_the_definition(R):
    for kind in ("random", "blocky"):
        p = U.planes_of(kind, 37, 45, seed=R)[0]
        opened, closed = U.fast(p, R, U.OPEN), U.fast(p, R, U.CLOSE)
        assert (opened <= p).all() and (p <= closed).all()                     # so the hats need no clamp
        assert np.array_equal(U.fast(opened, R, U.OPEN), opened) and np.array_equal(U.fast(closed, R, U.CLOSE), closed)   # idempotent
        assert np.array_equal(U.fast(p, R, U.TOPHAT), p - opened) and np.array_equal(U.fast(p, R, U.BOTHAT), closed - p)
        assert np.array_equal(U.fast(255 - p, R, U.MIN), 255 - U.fast(p, R, U.MAX))   # duality
        if R <= U.MEDIAN_RADIUS_MAX:
            med = U.fast(p, R, U.MEDIAN)
            assert (U.fast(p, R, U.MIN) <= med).all() and (med <= U.fast(p, R, U.MAX)).all()


def test_constant_plane_and_radius_zero():
    plane = U.random_planes(12, 17)[0]
    for one in (U.fast, U.brute):
        for code in U.CODES:
            want = np.zeros_like(plane) if code in (U.TOPHAT, U.BOTHAT) else plane
            assert np.array_equal(one(plane, 0, code), want), code
    for v in (0, 1, 128, 255):
        flat = np.full((9, 14), v, np.uint8)
        for code in U.CODES:
            want = np.zeros_like(flat) if code in (U.TOPHAT, U.BOTHAT) else flat
            assert np.array_equal(U.fast(flat, 3, code), want), (v, code)


def test_lower_median_and_the_byte_counter():
    """an even window takes the lower of the two middle samples; at R = 7 one bin can hold all 225 samples"""
    two = np.array([[10, 20]], np.uint8)
    assert U.fast(two, 1, U.MEDIAN).tolist() == [[10, 10]] == U.brute(two, 1, U.MEDIAN).tolist()
    assert (2 * U.MEDIAN_RADIUS_MAX + 1) ** 2 == 225 < 256
    split = U.split_planes(20, 40)[0]
    assert np.array_equal(U.fast(split, 3, U.MEDIAN), U.brute(split, 3, U.MEDIAN))


def test_expected_planes_follow_the_pairing_rule():
    src3, src1 = U.random_planes(9, 11, 3), U.random_planes(9, 11, 1)
    got = U.expected(src1, 3, 2, (U.COPY, U.OPEN, U.TOPHAT))
    assert np.array_equal(got[0], src1[0]) and np.array_equal(got[1], U.fast(src1[0], 2, U.OPEN)) and np.array_equal(got[2], U.fast(src1[0], 2, U.TOPHAT))
    got = U.expected(src3, 3, 1, (U.MEDIAN, U.COPY, U.MAX))
    assert np.array_equal(got[0], U.fast(src3[0], 1, U.MEDIAN)) and np.array_equal(got[1], src3[1]) and np.array_equal(got[2], U.fast(src3[2], 1, U.MAX))
    assert np.array_equal(U.expected(src3, 1, 1, (U.MIN, 9, 9))[0], U.fast(src3[0], 1, U.MIN))     # entries behind C_dst are ignored
    what = (U.MEDIAN, U.CLOSE, U.BOTHAT)
    assert all(np.array_equal(a, b) for a, b in zip(U.expected(src3, 3, 3, what, one=U.brute), U.expected(src3, 3, 3, what)))


def test_shared_integer_arithmetic_of_the_kernels(raw_lib):
    """rank_math.h compiled for the host: chains, band rows, the median's rank, and the walk over sixteen packed byte counters"""
    assert [raw_lib.cvh_debug_rank_chain(c) for c in U.CODES] == [-1, 0, 1, -1, 0, 1, 0, 1]
    assert [raw_lib.cvh_debug_rank_twice(c) for c in U.CODES] == [0, 0, 0, 0, 1, 1, 1, 1]
    for R in range(U.RADIUS_MAX + 1):
        rows = raw_lib.cvh_debug_rank_band_rows(R)
        assert rows == U.band_rows(R) and rows % (2 * R + 1) == 0 and U.BAND <= rows < U.BAND + 2 * R + 1
    fn = raw_lib.cvh_debug_rank_median_index
    fn.restype, fn.argtypes = ctypes.c_uint, [ctypes.c_uint]
    assert all(fn(n) == (n - 1) // 2 for n in range(1, 226))
    walk = raw_lib.cvh_debug_rank_walk
    walk.argtypes = [ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), ctypes.c_uint]
    rows = [[0] * 15 + [225], [225] + [0] * 15, [14] * 16, [0, 0, 112, 0, 0, 113] + [0] * 10]
    rows += [list(r) for r in (U.random_planes(8, 16, seed=5)[0] % 15).astype(int)]
    for counts in rows:
        words = (ctypes.c_uint * 4)(*[sum(counts[4 * q + b] << (8 * b) for b in range(4)) for q in range(4)])
        for start in (0, 3):
            for t in range(start, start + sum(counts) + 2):
                before = ctypes.c_uint(start)
                at = walk(words, ctypes.byref(before), t)
                cum = np.cumsum([start] + counts)
                want = next((i for i in range(16) if cum[i + 1] > t), 16)
                assert at == want and before.value == cum[want], (counts, start, t)


def test_the_propositions_on_the_cpu_oracle():
    """128 x 128, checkerboard start, default parameters, 600 steps at most; streams from synth.splitmix64_stream(11, ..)
    (rank_util.salt_image, rank_util.ramp_image).  Measured on the oracle (steps, IoU with the truth, better of mask / inverted mask):
        salt and pepper, raw     299   0.528
        median, R = 1            188   0.952
        median, R = 2            251   0.974
        ramp, raw                  4   0.130
        white top-hat, R = 10    600   1.000   (the cap is reached)
    The bars are the issue's; the inputs are fixed integers and the oracle is deterministic."""
    rows = {name: U.oracle_proposition(name) for name in U.PROPOSITIONS}
    for name, (_, steps, found) in rows.items():
        print(name, steps, round(found, 3))
    tophat = U.proposition_plane("ramp tophat R=10")
    print("top-hat's largest value", int(tophat.max()))
    assert (U.fast(np.array(U.ramp_image()), U.RAMP_R, U.OPEN) <= U.ramp_image()).all()
    assert rows["salt raw"][2] <= 0.6
    assert rows["salt median R=2"][2] >= 0.95
    assert rows["ramp raw"][2] <= 0.3
    assert rows["ramp tophat R=10"][2] >= 0.98
