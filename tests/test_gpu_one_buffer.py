"""Option "one_buffer" of the 2-pixel wave kernel (csv_wave2_ob_kernel, csv_wave2_body.inc with OB): 1 updates ONE padded level-set buffer
in place -- what a wave reads of cells another wave writes comes from the row pads and the strips' shadow rows, double-buffered by
iteration parity -- 0 is the ping-pong pair.  Which wave computes which pixel, every pixel's arithmetic and the order of every sum are
the same, so the two settings must agree BIT FOR BIT: level set, mask, region means and norm of every trace row, steps done.

Every case forces "kernel" = 3 and "resident" = 0.  Shapes are the smallest at which a path can go wrong: widths 144 and 160 (a full
wave-column and a short one), 272 (three wave-columns: lane 0's halo pair and the east extra both come from a neighbour's pad, the third
column's workgroup has an idle wave); five equal strips (odd: the last upper strip has no partner) of 1, 2, 3, 4, 5 and 9 rows with a
ragged last one -- shorter than the rows a strip publishes, shorter than the prologue's rows, exactly one group, an interior group
between the edge groups --; strips dealt by weight under the class-major numbering."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STRIP_ROWS = (1, 2, 3, 4, 5, 9)
WIDTHS = (144, 160, 272)
COUNTS = (1, 2, 3, 7, 33)     # odd and even: both parities are read back; 33 = two graphs + a plain launch


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def plane_for(h, w, seed):
    """A disk on a gradient plus noise: two regions with different means."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    disk = ((yy - h / 2.0) ** 2 * 4 + (xx - w / 2.0) ** 2 < (w / 3.0) ** 2) * 120.0
    return np.clip(40 + disk + xx * (30.0 / w) + rng.integers(0, 24, size=(h, w)), 0, 255).astype(np.uint8)


def start_for(capi, h, w, start):
    if start == "checkerboard":
        return capi.checkerboard_host(h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where((yy - 0.4 * h) ** 2 + (xx - 0.55 * w) ** 2 <= (0.3 * min(h, w)) ** 2, 1.0, -1.0)


def open_ctx(capi, plane, u0, ob, opts, trace, **pk):
    h, w = plane.shape
    ctx = capi.Context(h, w, 1, capi.make_params(**pk))
    for k, v in dict(math_mode=2, kernel=3, resident=0, trace=trace, **opts, one_buffer=ob).items():
        ctx.set_option(k, v)
    ctx.set_image([plane])
    ctx.set_levelset(u0)
    return ctx


def result(ctx, steps, done, nrm):
    return dict(u=ctx.get_levelset(), mask=ctx.get_mask(), means=ctx.get_means(), trace=ctx.get_trace(steps), done=done, norm=nrm)


def run_once(capi, plane, u0, ob, opts, steps, chosen=None, **pk):
    with open_ctx(capi, plane, u0, ob, opts, steps, **pk) as ctx:
        info = ctx.launch_info()
        if chosen is None:
            chosen = ob
        assert info["one_buffer"] == str(chosen), info
        assert info["kernel"].startswith("csv_wave2_ob_kernel<" if chosen else "csv_wave2_kernel<1, true, 3, "), info
        done, nrm = ctx.run(steps)
        return result(ctx, steps, done, nrm)


def assert_same_bits(a, b, what):
    assert a["done"] == b["done"], (what, a["done"], b["done"])
    assert a["u"].dtype == np.float64 and np.array_equal(a["u"], b["u"]), (what, int((a["u"] != b["u"]).sum()), np.argwhere(a["u"] != b["u"])[:8])
    assert np.array_equal(a["mask"], b["mask"]), what
    assert np.array_equal(a["means"][0], b["means"][0]) and np.array_equal(a["means"][1], b["means"][1]), (what, a["means"], b["means"])
    assert a["trace"].shape == b["trace"].shape and np.array_equal(a["trace"], b["trace"]), (what, a["trace"], b["trace"])
    assert a["norm"] == b["norm"], what
    assert np.isfinite(a["u"]).all() and np.isfinite(a["trace"]).all(), what


def both(capi, plane, u0, opts, steps, what, **pk):
    one = run_once(capi, plane, u0, 1, opts, steps, **pk)
    pair = run_once(capi, plane, u0, 0, opts, steps, **pk)
    assert_same_bits(one, pair, what)
    return one


def equal_strips(sr):
    return 4 * sr + max(1, sr // 2), dict(wave_cls=0, strip_rows=sr)


@pytest.mark.parametrize("start", ["checkerboard", "disk"])
@pytest.mark.parametrize("regime", ["far", "near"])
def test_short_strips_same_bits(capi, regime, start):
    """Strips of 1 .. 9 rows x the three widths, 1 .. 33 iterations, in the far regime (dt = 1: |u| leaves the near field within two
    iterations) and the all-near regime (dt = 0.001: the near-form march), from the checkerboard and from a disk."""
    pk = dict(tol=0.0, dt=0.001 if regime == "near" else 1.0)
    for i, sr in enumerate(STRIP_ROWS):
        h, opts = equal_strips(sr)
        for j, steps in enumerate(COUNTS):
            w = WIDTHS[(i + j) % 3]
            plane, u0 = plane_for(h, w, 1000 * sr + w), start_for(capi, h, w, start)
            r = both(capi, plane, u0, opts, steps, (sr, w, steps, regime, start), **pk)
            assert r["done"] == steps


@pytest.mark.parametrize("w", WIDTHS)
def test_every_width_at_every_strip_length(capi, w):
    """The widths not met above at a strip length, 7 iterations (both parities written and read)."""
    for sr in STRIP_ROWS:
        h, opts = equal_strips(sr)
        both(capi, plane_for(h, w, 7 * sr + w), capi.checkerboard_host(h, w), opts, 7, (sr, w), tol=0.0)


@pytest.mark.parametrize("h,w,opts", [(1000, 144, dict(strips=90, wave_sync=1)), (1024, 1008, {}), (531, 272, dict(strips=33))])
def test_strips_dealt_by_weight_same_bits(capi, h, w, opts):
    """The class-major numbering with strips dealt by cumulative weight (the two strips of a workgroup differ in length), an odd strip
    count, and 1024 x 1008 in the automatic geometry: nine wave-columns, more than one workgroup per CU."""
    both(capi, plane_for(h, w, 77), capi.checkerboard_host(h, w), opts, 7, (h, w), tol=0.0)


def test_two_enqueues_without_a_sync(capi):
    """16 + 18 steps enqueued back to back (a graph, then two plain launches and a graph), one sync."""
    sr, w = 5, 272
    h, opts = equal_strips(sr)
    plane, u0 = plane_for(h, w, 3), capi.checkerboard_host(h, w)
    out = {}
    for ob in (1, 0):
        with open_ctx(capi, plane, u0, ob, opts, 34, tol=0.0) as ctx:
            assert ctx.launch_info()["one_buffer"] == str(ob)
            ctx.enqueue_steps(16)
            ctx.enqueue_steps(18)
            done, nrm, stopped = ctx.sync()
            assert done == 34 and not stopped
            out[ob] = result(ctx, 34, done, nrm)
    assert_same_bits(out[1], out[0], "16 + 18")


@pytest.mark.parametrize("parity", [0, 1])
def test_a_run_that_may_stop_keeps_the_pair(capi, parity):
    """tol > 0: the flow is NOT chosen (chain mode computes one iteration beside the stop rule, which one buffer would not survive) --
    launch_info says so, and the run is the pair's: same stop iteration, on an even and on an odd one, same level set."""
    sr, w = 5, 272
    h, opts = equal_strips(sr)
    plane, u0 = plane_for(h, w, 5), capi.checkerboard_host(h, w)
    free = run_once(capi, plane, u0, 0, opts, 12, tol=0.0)
    norms = free["trace"][:, -1]
    k = next((i for i in range(2, 11) if i % 2 == parity and norms[i] < norms[:i].min()), None)
    assert k is not None, norms
    tol = float(np.sqrt(norms[k] * norms[:k].min()) / np.sqrt((plane.astype(np.float64) ** 2).sum()))
    asked = run_once(capi, plane, u0, 1, opts, 12, chosen=0, tol=tol)
    pair = run_once(capi, plane, u0, 0, opts, 12, tol=tol)
    assert_same_bits(asked, pair, ("stop", k))
    assert asked["done"] == k + 1, (asked["done"], k, norms)


def test_set_run_get_round_trips(capi):
    """set_levelset -> steps -> get_levelset / get_mask at a width whose rows are padded, twice on one context (a new level set ends the
    flow's hold on the old one), with a read-back between two enqueues (the mirror is refreshed, the slab stays the master)."""
    sr, w = 3, 160
    h, opts = equal_strips(sr)
    plane = plane_for(h, w, 11)
    starts = [capi.checkerboard_host(h, w), start_for(capi, h, w, "disk") * 2.5]
    out = {}
    for ob in (1, 0):
        with open_ctx(capi, plane, starts[0], ob, opts, 8, tol=0.0) as ctx:
            got = []
            assert np.array_equal(ctx.get_levelset(), starts[0])
            for u0 in starts:
                ctx.set_levelset(u0)
                ctx.enqueue_steps(3)
                ctx.sync()
                got += [ctx.get_mask(), ctx.get_levelset()]        # after an odd number of steps
                ctx.enqueue_steps(2)
                ctx.sync()
                got += [ctx.get_levelset(), ctx.get_mask(), ctx.get_means()[0]]
            out[ob] = got
    for a, b in zip(out[1], out[0]):
        assert np.array_equal(a, b)
    assert not np.array_equal(out[1][1], out[1][2])
