"""Facts about the numpy restatement of the four-phase iteration (multiphase_util.py; include/chanvese_hip.h, "Four phases") that the
GPU comparison rests on: its symmetries, what the channel sum means, and -- the conditioning check -- how far apart two summation
orders end after every GPU case's iterations.  No device."""
import numpy as np
import pytest

import multiphase_util as M
import np_restatement as R


def test_swapping_a_and_b_swaps_the_results():
    planes, u1, u2 = M.case_inputs(24, 64, 1)
    a1, a2, _, ta = M.run(planes, u1, u2, M.OTHER_A, M.OTHER_B, 4)
    b2, b1, _, tb = M.run(planes, u2, u1, M.OTHER_B, M.OTHER_A, 4)
    assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
    # rows: c11 c10 c01 c00 n1 n2 -> c11 c01 c10 c00 n2 n1 (the sums of the swapped products are the same numbers: w10 <-> w01)
    assert np.array_equal(ta[:, [0, 2, 1, 3, 5, 4]], tb)


def test_identical_starts_with_identical_parameters_stay_identical():
    planes, u1, _ = M.case_inputs(24, 64, 1)
    v1, v2, _, trace = M.run(planes, u1, u1.copy(), M.OTHER_A, M.OTHER_A, 5)
    assert np.array_equal(v1, v2)
    assert np.array_equal(trace[:, 1], trace[:, 2]) and np.array_equal(trace[:, 4], trace[:, 5])


def test_channel_sum_is_what_the_formula_says():
    """C = 3 with lambda = (1, 0, 0): the level sets of the one-channel run on plane 0 with 1/3 in the fit term -- dt / 3 on the region
    term, i.e. the one-channel run with every lambda 1/3"""
    planes, u1, u2 = M.case_inputs(24, 64, 3)
    three = dict(M.DEFAULT, lambda1=(1.0, 0.0, 0.0), lambda2=(1.0, 0.0, 0.0))
    one = dict(M.DEFAULT, lambda1=(1.0 / 3,), lambda2=(1.0 / 3,))
    a1, a2, _, ta = M.run(planes, u1, u2, three, three, 4)
    b1, b2, _, tb = M.run(planes[:1], u1, u2, one, one, 4)
    scale = max(1.0, np.abs(b1).max(), np.abs(b2).max())
    assert np.abs(a1 - b1).max() <= 1e-12 * scale and np.abs(a2 - b2).max() <= 1e-12 * scale   # ((q / 3) vs (q * (1/3)): roundings apart)
    assert np.allclose(ta[:, [0, 3, 6, 9]], tb[:, :4], rtol=1e-12, atol=0) and np.allclose(ta[:, -2:], tb[:, -2:], rtol=1e-12, atol=0)


def test_means_of_a_hard_partition_are_the_class_means():
    """eps -> 0: the weights become indicators and c_ab the plain means of the four sign classes"""
    planes, cls = M.disks_image(32, 48, 1, noise=0.0)
    u1 = np.where(cls & 1, 1.0, -1.0)
    u2 = np.where(cls & 2, 1.0, -1.0)
    c = M.means(planes, u1, u2, eps=1e-9)
    assert np.allclose(c[:, 0], [M.LEVELS[3], M.LEVELS[1], M.LEVELS[2], M.LEVELS[0]], rtol=1e-6)


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_conditioning_of_every_gpu_case(case):
    """the pairwise-sum form and the fsum form agree after the case's iterations to 1e-11 relative in every mean and norm and to
    1e-11 max(1, max|phi|) in both level sets: two decades below the GPU tolerance.  And the restatement's own level sets keep the
    label comparison meaningful: at most 0.1 % of the pixels within 1e-6 of a zero."""
    h, w, C, which = case
    planes, u1, u2 = M.case_inputs(h, w, C)
    pa, pb = M.params_of(which)
    v1, v2, steps, trace = M.case_reference(case)
    x1, x2, xsteps, xtrace = M.run(planes, u1, u2, pa, pb, M.ITERATIONS, total=M.exact)
    assert steps == xsteps == M.ITERATIONS
    rel = np.abs(trace - xtrace) / np.abs(xtrace)
    scale = max(1.0, np.abs(x1).max(), np.abs(x2).max())
    e1, e2 = np.abs(v1 - x1).max() / scale, np.abs(v2 - x2).max() / scale
    share = M.near_zero(v1, v2).mean()
    print(M.case_id(case), "trace", rel.max(), "phi1", e1, "phi2", e2, "near-zero share", share)
    assert np.isfinite(trace).all() and rel.max() <= 1e-11
    assert e1 <= 1e-11 and e2 <= 1e-11
    assert share <= 1e-3


def test_stop_case_exists():
    tol, k = M.stop_case()
    assert 2 < k < 16 and tol > 0
    planes, _, _ = M.case_inputs(*M.STOP_SHAPE)
    assert R.stop_condition(planes, tol) > 0
