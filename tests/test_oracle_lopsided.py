"""The labels of tests/lopsided_util.py, checked on the oracle (CPU): what tests/test_gpu_lopsided.py asserts at 1e-9 is defined by the
reference's own arithmetic to 1e-11, what it only records is not, and the saturated cases are 0 / 0 in the reference itself."""
import numpy as np
import pytest

import lopsided_util as L
import np_restatement as R
from test_gpu_param_edges import conditioned
import test_gpu_param_edges as T


def _first_iterate(oracle, planes, u0, pk):
    return oracle.csv_run(planes, u0, oracle.make_params(**pk), 1)[0]


@pytest.mark.parametrize("flavour", L.NAMES)
def test_conditioned_cases_have_100x_headroom(oracle, flavour):
    """Both level sets whose means the two trace rows of the GPU test hold (u0 and the first iterate): the oracle within 1e-11 of the
    long-double means, 1/100 of the 1e-9 bar; the numpy restatement within its usual 1e-12 of the oracle."""
    channels = L.SHAPES[flavour][1]
    planes = L.image(flavour)
    for case in L.conditioned_cases(flavour) + L.FAR_CONDITIONED:
        pk = L.params(channels, eps=case["eps"])
        u0 = L.case_start(flavour, case)
        for u in (u0, _first_iterate(oracle, planes, u0, pk)):
            err = L.reference_error(oracle, planes, u, case["eps"])
            assert err.max() <= 1e-11, (flavour, case, err)
        c1, c2 = oracle.region_means(planes, u0, case["eps"])
        for k, pl in enumerate(planes):
            assert abs(R.region_mean(pl, u0, True, case["eps"]) / c1[k] - 1) <= 1e-12, (flavour, case, k)
            assert abs(R.region_mean(pl, u0, False, case["eps"]) / c2[k] - 1) <= 1e-12, (flavour, case, k)
        if flavour == "state32":
            assert case["R"] <= 1e4 or case in L.FAR_CONDITIONED


def test_covering_design():
    """Every (minority, side), every R and every eps meets every flavour, in at most 12 cases."""
    for flavour in L.NAMES:
        cases = L.conditioned_cases(flavour)
        assert len(cases) <= 12
        assert {(c["minority"], c["side"]) for c in cases} == {(m, s) for m in (1, 3, "row") for s in (1, -1)}
        assert {c["R"] for c in cases} == ({1e2, 1e4} if flavour == "state32" else {1e2, 1e4, 1e6})
        assert {c["eps"] for c in cases} == {0.25, 4.0}


@pytest.mark.parametrize("flavour", L.NAMES)
def test_ill_conditioned_cases_are_beyond_the_bar(oracle, flavour):
    """No minority pixel: the reference's empty-side mean is further than 1e-9 from the long-double value (not assertable at 1e-9), the
    majority side's is defined to 1e-11 (assertable)."""
    planes = L.image(flavour)
    for case in L.ILL_CASES:
        u0 = L.case_start(flavour, case)
        err = L.reference_error(oracle, planes, u0, case["eps"])
        e = L.empty_region(case["side"])
        assert err[e].min() > 1e-9 and np.isfinite(err[e]).all(), (flavour, case, err)
        assert err[1 - e].max() <= 1e-11, (flavour, case, err)
    for case in L.MARGINAL_CASES:
        err = L.reference_error(oracle, planes, L.case_start(flavour, case), case["eps"])
        assert err[1 - L.empty_region(case["side"])].max() <= 1e-11, (flavour, case, err)


def test_marginal_cases_have_no_headroom(oracle):
    """|u| = 1e7 eps and 1e9 eps without a minority pixel: the empty side's mean of the reference is not 100 x inside the 1e-9 bar (so the
    GPU test does not assert it) and not beyond the bar in every case either (so the cases are not labelled ill-conditioned)."""
    for R in (1e7, 1e9):
        errs = [L.reference_error(oracle, L.image(f), L.case_start(f, c), c["eps"])[L.empty_region(c["side"])].max()
                for f in L.NAMES for c in L.MARGINAL_CASES if c["R"] == R]
        assert max(errs) > 1e-11 and min(errs) <= 1e-9, (R, errs)


@pytest.mark.parametrize("flavour", L.NAMES)
def test_saturated_cases_are_nan_in_the_reference(oracle, flavour):
    planes = L.image(flavour)
    for case in L.SATURATED:
        c = np.array(oracle.region_means(planes, L.case_start(flavour, case), case["eps"]))
        e = L.empty_region(case["side"])
        assert np.isnan(c[e]).all() and np.isfinite(c[1 - e]).all(), (flavour, case, c)


@pytest.mark.parametrize("flavour", L.NAMES)
def test_collapsing_case(oracle, flavour, monkeypatch):
    """The inside vanishes inside the window; at the three compared iterations a 1-ulp perturbation of u0 moves the oracle by less than
    1e-11 of max|u| (the `conditioned` recipe of tests/test_gpu_param_edges.py) and its means are defined to 1e-11."""
    planes, u0, pk = L.flavour_collapse(flavour)
    counts = L.inside_counts(oracle, planes, u0, pk, L.COLLAPSE_STEPS)
    two, empty, end = L.collapse_checkpoints(counts)
    assert L.COLLAPSE_WINDOW[0] <= empty <= L.COLLAPSE_WINDOW[1] and counts[empty - 2] > 0, counts
    assert two < empty < end and all(c == 0 for c in counts[empty - 1:]), counts
    monkeypatch.setattr(T, "CHECKPOINTS", (two, empty, end))
    cond = conditioned(oracle, planes, u0, pk)
    assert max(cond.values()) < 1e-11, cond
    for s in (two, empty, end):
        u = oracle.csv_run(planes, u0, oracle.make_params(**pk), s - 1)[0] if s > 1 else u0
        assert L.reference_error(oracle, planes, u, pk["eps"]).max() <= 1e-11, (flavour, s)
