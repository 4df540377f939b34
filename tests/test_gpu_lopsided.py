"""Every CSV flavour on level sets with a nearly or wholly empty region (tests/lopsided_util.py), against the oracle.

There the FAST flavours' centred sums (sum (H - 1/2), shifted back by N/2; complements N - sum H; chain mode: rounded to 64-bit fixed
point at a scale sized for N/2) obtain a sum of a few pixels as the small difference of two numbers of size N/2.  Flavours, shapes
and the launch_info() pin are those of tests/test_gpu_param_edges.py; the band of every case is labelled from the oracle on the CPU
(tests/test_oracle_lopsided.py), never from what the GPU gives.

(a) conditioned: 1, 3 or a row of minority pixels, |u| = 1e2 .. 1e6 eps (and three pixels at 1e12 eps): 2 iterations, the suite's bars
    (check() of tests/test_gpu_param_edges.py): every trace entry rtol 1e-9, level set 1e-9 max|u|, mask, steps_done.
(b) a run whose inside vanishes (nu > 0): the same bars at the last iteration with two or more inside pixels, the first with none, the end.
(c) no minority pixel, |u| = 1e7, 1e9 (marginal) and 1e12 eps (ill-conditioned): the bars on what the reference still defines -- level set,
    norm, mask, steps_done, the majority side's mean; the empty side's mean is printed beside the reference's own error.
(d) saturated, |u| = 1e18 eps: the empty side's mean is 0 / 0 in the reference; NaN for NaN, pixel for pixel.
(e) 2048^2 resident and 4096^2 chain mode with three minority pixels: where the absolute error of the centred sums would show."""
import numpy as np
import pytest

import lopsided_util as L
import param_edges_util as E
from test_gpu_param_edges import FLAVOURS, check, oracle_run, run_single

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def balanced_member():
    """The member beside the lop-sided one in run_batch: signed-distance start on a noisy disk, default parameters."""
    (h, w), _ = L.SHAPES["batch"]
    return E.image("disk", h, w, 1, seed=77), E.start(None, "sdist", h, w, 1.0), L.params(1)


def run_in_batch(capi, members, s):
    """[(u, done, trace, mask)] of the members [(planes, u0, pk)] of one run_batch of at most s iterations."""
    (h, w), _ = L.SHAPES["batch"]
    ctxs = []
    try:
        for planes, u0, pk in members:
            c = capi.Context(h, w, 1, capi.make_params(**pk))
            ctxs.append(c)
            c.set_option("trace", s)
            c.set_image(planes)
            c.set_levelset(u0)
            # a member's own flow (what it would run alone); in the batch every member runs the fused kernel
            assert c.launch_info()["kernel"].startswith(("csv_wave", "csv_resident")), c.launch_info()
        out = capi.run_batch(ctxs, s)
        return [(c.get_levelset(), out[i][0], c.get_trace(out[i][0]), c.get_mask()) for i, c in enumerate(ctxs)]
    finally:
        for c in ctxs:
            c.close()


def run_flavour(capi, oracle, flavour, planes, u0, pk, s):
    if flavour != "batch":
        return run_single(capi, flavour, planes, u0, pk, s)
    other = balanced_member()
    got, got2 = run_in_batch(capi, [(planes, u0, pk), other], s)
    check(oracle, ("batch", "balanced", "sdist", "disk", s), other[0], other[1], other[2], s, got2)
    return got


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_launch_geometry_is_the_one_the_seams_come_from(capi, flavour):
    """The minority pixels sit on strip, tile and wave-column seams computed on the host (lopsided_util.geometry): launch_info() of the
    flavour's context reports that very kernel and grid."""
    (h, w), channels, opts, prefix, math = FLAVOURS[flavour]
    g = L.geometry(flavour)
    with capi.Context(h, w, channels, capi.make_params(**L.params(channels))) as ctx:
        for key, v in opts.items():
            ctx.set_option(key, v)
        ctx.set_image(L.image(flavour))
        ctx.set_levelset(L.case_start(flavour, L.conditioned_cases(flavour)[0]))
        info = ctx.launch_info()
    assert info["kernel"].startswith(prefix) and info.get("math", math) == math, info
    assert int(info["data_flow"]) == g["kind"], (info, g)
    if g["kind"] == 4:
        assert (int(info["tiles_x"]), int(info["tiles_y"]), int(info["tile_rows"])) == (g["tiles_x"], g["tiles_y"], g["strip_rows"]), (info, g)
    else:
        assert (int(info["wave_columns"]), int(info["strips"]), int(info["strip_rows"])) == (g["tiles_x"], g["tiles_y"], g["strip_rows"]), (info, g)
    first, last, seam = L.seams(flavour)
    assert seam[0] in g["rows"][1:-1] and (g["tiles_x"] == 1 or seam[1] % g["cols"] == 0), (seam, g)


# ---- (a)

CONDITIONED = [(f, i) for f in L.NAMES for i in range(len(L.conditioned_cases(f)) + len(L.FAR_CONDITIONED))]


@pytest.mark.parametrize("flavour,i", CONDITIONED)
def test_conditioned_band(capi, oracle, flavour, i):
    """Trace row 0: the means the initial-sums kernel produced; row 1: the means from the fused step's own sums of u_1, still lop-sided
    (delta_eps is tiny out there)."""
    channels = L.SHAPES[flavour][1]
    case = (L.conditioned_cases(flavour) + L.FAR_CONDITIONED)[i]
    pk = L.params(channels, eps=case["eps"])
    planes, u0 = L.image(flavour), L.case_start(flavour, case)
    f32 = flavour == "state32"
    if f32:
        u0 = u0.astype(np.float32).astype(np.float64)
    what = (flavour, "%s/%+d/%g/%g" % (case["minority"], case["side"], case["R"], case["eps"]), "lopsided", "disk", 2)
    got = run_flavour(capi, oracle, flavour, planes, u0, pk, 2)
    assert got[1] == 2 and got[2].shape == (2, 2 * channels + 1), what
    check(oracle, what, planes, u0, pk, 2, got, float_state=f32)


# ---- (b)

@pytest.mark.parametrize("flavour", L.NAMES)
def test_inside_vanishes_during_the_run(capi, oracle, flavour):
    planes, u0, pk = L.flavour_collapse(flavour)
    counts = L.inside_counts(oracle, planes, u0, pk, L.COLLAPSE_STEPS)
    f32 = flavour == "state32"
    if f32:
        u0 = u0.astype(np.float32).astype(np.float64)
    for s in L.collapse_checkpoints(counts):
        what = (flavour, "collapse", "sdist", "disk140", s)
        if flavour != "batch":
            got = run_single(capi, flavour, planes, u0, pk, s)
        else:   # beside a member that stops on its own tolerance while the other's inside vanishes
            img2, u2, pk2 = balanced_member()
            norms = oracle.csv_run(img2, u2, oracle.make_params(**pk2), s)[3][:, -1]
            k = next(k for k in range(3, s) if norms[k - 1] < norms[:k - 1].min() * (1 - 1e-5))
            pk2 = dict(pk2, tol=norms[k - 1] / oracle.stop_condition(img2, 1.0) * (1 + 1e-6))
            got, got2 = run_in_batch(capi, [(planes, u0, pk), (img2, u2, pk2)], s)
            assert got2[1] == k and 1 < k < s, (got2[1], k, s)
            check(oracle, ("batch", "stops", "sdist", "disk", s), img2, u2, pk2, s, got2)
        assert got[1] == s
        check(oracle, what, planes, u0, pk, s, got, float_state=f32)
    if not f32:
        assert not got[3].any()          # the mask at the end: nothing inside


# ---- (c)

def check_defined(oracle, what, planes, u0, pk, s, got, side, float_state):
    """What the reference still defines without a minority pixel; returns (empty side's means of row 0: GPU, oracle)."""
    u_g, done_g, tr_g, m_g = got
    u_c, done_c, tr_c = oracle_run(oracle, planes, u0, pk, s, float_state)
    nc = len(planes)
    assert done_g == done_c == s and tr_g.shape == tr_c.shape, (what, done_g, done_c)
    err = float(np.abs(u_g - u_c).max() / np.abs(u_c).max())
    assert err <= (2e-5 if float_state else 1e-9), (what, err)      # FP32 state: the bar of tests/test_gpu_state32.py past iteration 1
    assert np.array_equal(m_g, oracle.mask(u_c)), what
    rows = slice(0, 1) if float_state else slice(0, s)              # FP32 state compares the first iteration's trace (test_gpu_param_edges.check)
    e = L.empty_region(side)
    majority = list(range((1 - e) * nc, (1 - e) * nc + nc)) + [2 * nc]
    assert np.allclose(tr_g[rows][:, majority], tr_c[rows][:, majority], rtol=1e-9, atol=0), (what, tr_g, tr_c)
    return tr_g[0, e * nc:(e + 1) * nc], tr_c[0, e * nc:(e + 1) * nc]


@pytest.mark.parametrize("flavour", L.NAMES)
def test_empty_region_marginal_and_ill_conditioned(capi, oracle, flavour):
    """The empty side has lambda = 0 (lopsided_util.ILL_CASES: the norm would otherwise inherit that mean's error).  Its mean is printed,
    not asserted: `pytest -s` shows the rows of the table in DESIGN section 5."""
    channels = L.SHAPES[flavour][1]
    planes = L.image(flavour)
    f32 = flavour == "state32"
    for case in L.MARGINAL_CASES + L.ILL_CASES:
        pk = L.ill_params(channels, case["side"])
        u0 = L.case_start(flavour, case)
        if f32:
            u0 = u0.astype(np.float32).astype(np.float64)
        what = (flavour, "empty/%+d/%g" % (case["side"], case["R"]))
        got = run_flavour(capi, oracle, flavour, planes, u0, pk, 2)
        c_g, c_o = check_defined(oracle, what, planes, u0, pk, 2, got, case["side"], f32)
        c_l = np.array(L.means_longdouble(planes, u0, case["eps"]))[L.empty_region(case["side"])]
        print("LOPSIDED-C %-12s R=%g side=%+d c_ld=%.15g c_ref=%.15g c_gpu=%.15g err_ref=%.2e err_gpu=%.2e" % (
            flavour, case["R"], case["side"], c_l[0], c_o[0], c_g[0], np.abs(c_o / c_l - 1).max(), np.abs(c_g / c_l - 1).max()))


# ---- (d)

@pytest.mark.parametrize("flavour", L.NAMES)
def test_saturated(capi, oracle, flavour):
    channels = L.SHAPES[flavour][1]
    planes = L.image(flavour)
    f32 = flavour == "state32"
    for case in L.SATURATED:
        pk = L.params(channels, tol=1e-3)
        u0 = L.case_start(flavour, case)
        if f32:
            u0 = u0.astype(np.float32).astype(np.float64)
        u_c, done_c, tr_c = oracle_run(oracle, planes, u0, pk, 3, f32)
        e = L.empty_region(case["side"])
        assert np.isnan(tr_c[0, e * channels:(e + 1) * channels]).all(), tr_c     # the reference's 0 / 0
        u_g, done_g, tr_g, m_g = run_flavour(capi, oracle, flavour, planes, u0, pk, 3)
        what = (flavour, case["side"], done_g, done_c, tr_g, tr_c)
        assert done_g == done_c, what
        assert tr_g.shape == tr_c.shape and np.array_equal(np.isnan(tr_g), np.isnan(tr_c)), what
        assert np.array_equal(np.isfinite(u_g), np.isfinite(u_c)), what[:4]
        assert np.array_equal(m_g, oracle.mask(u_c)), what[:4]        # no finite garbage where the reference has NaN


# ---- (e)

@pytest.mark.parametrize("n,opts,prefix", [(2048, dict(resident=1), "csv_resident_kernel<"),
                                           (4096, dict(kernel=3, resident=0), "csv_wave2_kernel<1, true, 3, ")])
def test_three_minority_pixels_at_scale(capi, oracle, n, opts, prefix):
    """Three inside pixels (first strip, mid-plane, last strip) among n^2 at |u| = 1e4 eps: sum H = 3 + n^2 / (1e4 pi) is obtained from
    sums of size n^2 / 2, whose stated agreement with exact sums (1e-13 of their own size) is 1e-6 absolute at 4096^2
    -- and 1e-9 of 537 is 5e-7.  Two iterations against the exact-sum oracle (on these inputs the reference-order sums agree with it to
    2.4e-13, measured on the CPU), c1 and c2 of both trace rows at rtol 1e-9."""
    planes = [E.synth.disk(n, 200, 50, noise=12, seed=n)]
    rng = np.random.default_rng(n)
    u0 = -1e4 * (1 + rng.uniform(-0.1, 0.1, size=(n, n)))
    for p in ((2, 5), (n // 2, n // 2 + 1), (n - 3, n - 6)):
        u0[p] = -u0[p]
    pk = L.params(1)
    with capi.Context(n, n, 1, capi.make_params(**pk)) as ctx:
        for key, v in opts.items():
            ctx.set_option(key, v)
        ctx.set_option("trace", 2)
        ctx.set_image(planes)
        ctx.set_levelset(u0)
        info = ctx.launch_info()
        assert info["kernel"].startswith(prefix) and info["chain"] == "1", info
        done, _ = ctx.run(2)
        tr_g = ctx.get_trace(2)
    assert done == 2
    p, u, tr_e = oracle.make_params(**pk), u0.copy(), []
    for _ in range(2):
        nrm, c1, c2 = oracle.csv_step_exact(planes, u, p)
        tr_e.append([c1[0], c2[0], nrm])
    tr_e = np.array(tr_e)
    print("scale", n, "c1, c2 relative to the exact-sum oracle:", np.abs(tr_g[:, :2] / tr_e[:, :2] - 1).max(axis=0))
    assert np.allclose(tr_g[:, :2], tr_e[:, :2], rtol=1e-9, atol=0), (tr_g, tr_e)
