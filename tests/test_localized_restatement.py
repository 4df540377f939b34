"""Facts about the numpy restatement of the localised-regions definition (localized_util.py) that the GPU tests rest on: the box sums,
the 64-bit bound, the demonstration, and the perturbation bound the GPU tolerance is."""
import numpy as np
import pytest

import localized_util as L


@pytest.mark.parametrize("shape,rad", [((5, 7), 1), ((9, 4), 3), ((6, 6), 127)])
def test_box_sums_equal_the_double_loop(shape, rad):
    rng = np.random.default_rng(7)
    x = rng.integers(0, L.ONE + 1, size=shape, dtype=np.uint64) * rng.integers(0, 256, size=shape, dtype=np.uint64)
    got, want = L.box_sums(x, rad), L.box_sums_brute(x, rad)
    assert all(int(got[r, c]) == want[r, c] for r in range(shape[0]) for c in range(shape[1]))
    counts = L.box_sums(np.ones(shape, dtype=np.uint64), rad)
    assert np.array_equal(counts, L.window_counts(shape[0], shape[1], rad))


def test_the_largest_window_sum_fits_64_bits():
    """wq = 2^40 everywhere, bytes 255, R = 127 on 260 x 260 (the plane's cumulative sums wrap; the window sums do not)"""
    h = w = 260
    x = np.full((h, w), L.ONE * 255, dtype=np.uint64)
    got = L.box_sums(x, 127)
    n = L.window_counts(h, w, 127)
    assert int(n.max()) == 255 * 255
    for r, c in ((0, 0), (130, 130), (259, 3), (127, 200)):
        assert int(got[r, c]) == int(n[r, c]) * 255 * L.ONE
    assert int(got.max()) == 65025 * 255 * L.ONE < 2 ** 64
    assert all(int(v) == int(k) * 255 * L.ONE for v, k in zip(got.ravel().tolist(), n.ravel().tolist()))


def test_demonstration_on_the_cpu():
    planes, disk, u = L.demo_inputs()
    local = L.iou(L.mask(L.demo_reference()), disk)
    glob = L.iou(L.mask(L.global_run(planes, u, L.DEFAULT, L.DEMO_STEPS)), disk)
    print("IoU localised R = 10, mu = 100:", local, "global:", glob)
    assert local >= 0.95
    assert glob <= 0.5


def test_the_perturbation_bound():
    worst = {L.case_id(c): L.perturbed_distance(c) for c in L.CASES}
    print(worst, "tolerance", L.tolerance())
    assert L.tolerance() == 10.0 * max(worst.values())
    assert 0.0 < L.tolerance() <= 1e-7


def test_the_cases_are_what_they_claim():
    assert L.geometry(L.SEAM_H, 130, L.SEAM_R)[3] == L.SEAM_H - 1
    cols, item_rows, _, strip = L.geometry(L.ITEM_H, 70, L.ITEM_R)
    assert strip == L.ITEM_H - 1 and strip == 3 * item_rows
    for case in L.CASES:
        ref, steps, trace = L.case_reference(case)
        assert steps == L.ITERATIONS and np.isfinite(ref).all() and np.isfinite(trace).all() and (trace > 0).all(), L.case_id(case)
    tol, k = L.stop_case()
    assert 2 < k < 16 and tol > 0
