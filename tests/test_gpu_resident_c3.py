"""Resident mode with three channels (csv_resident_kernel<3, NRT>, option "resident" = 1): the colour counterpart of
tests/test_gpu_resident.py.  Same parity bar as the one-channel resident flow and the three-channel per-launch flow: level set, every
trace row (c1_0..2, c2_0..2, norm), means <= 1e-9 against the oracle, identical stop iteration, mask equal; plus chunk boundaries,
continuation into the per-launch flow and back, the straight-line flavours and the release-line sharing bit for bit, the near regime,
and the planes that do not qualify.  resident_ctx() asserts that the three-channel resident kernel is what runs: no test here can
silently exercise the per-launch flow."""
import numpy as np
import pytest

from chan_vese_amd import synth

pytestmark = pytest.mark.gpu

LAM = dict(lambda1=[1, 0.8, 0.5], lambda2=[0.7, 0.5, 1])          # per-channel weights (test_csv_three_channel_two_pixel_kernel's)


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def rel_err(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def resident_ctx(capi, h, w, pk):
    ctx = capi.Context(h, w, 3, capi.make_params(**pk))
    ctx.set_option("resident", 1)
    info = ctx.launch_info()
    assert info["kernel"].startswith("csv_resident_kernel<3"), info     # the three-channel resident kernel, not a per-launch flow
    return ctx, info


def colour_disk(h, w, noise=14, seed=7):
    """[B, G, R] planes of a noisy disk: another foreground / background pair and another noise seed per channel."""
    n = max(h, w)
    return [synth.disk(n, fg, bg, noise=noise, seed=seed + k, h=h, w=w) for k, (fg, bg) in enumerate(((200, 50), (90, 160), (230, 120)))]


@pytest.mark.parametrize("shape", [(16, 16), (16, 128), (32, 256), (48, 130), (96, 160), (96, 128), (130, 258), (200, 384), (256, 1024), (666, 500)])
def test_resident_c3_small_shapes(capi, oracle, shape):
    h, w = shape
    rng = np.random.default_rng(3 * h + w)
    planes = [rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(3)]
    u0 = oracle.checkerboard(h, w)
    pk = dict(tol=0, nu=0.01, dt=0.5, **LAM)
    for steps in (1, 2, 9):
        u_c, _, nrm_c, tr_c = oracle.csv_run(planes, u0, oracle.make_params(**pk), steps)
        ctx, info = resident_ctx(capi, h, w, pk)
        with ctx:
            ctx.set_option("trace", steps)
            ctx.set_image(planes)
            ctx.set_levelset(u0)
            done, nrm = ctx.run(steps)
            u_g, tr_g, m_g = ctx.get_levelset(), ctx.get_trace(steps), ctx.get_mask()
            c1g, c2g = ctx.get_means()
        assert done == steps, (shape, steps, done, info)
        print("c3 small", shape, steps, "rel_err", rel_err(u_g, u_c), "trace", float(np.abs(tr_g / tr_c - 1).max()))
        assert rel_err(u_g, u_c) <= 1e-9, (shape, steps, rel_err(u_g, u_c), info)
        assert tr_g.shape == tr_c.shape == (steps, 7)
        assert np.allclose(tr_g, tr_c, rtol=1e-9, atol=0), (shape, steps)
        assert nrm == pytest.approx(nrm_c, rel=1e-9)
        assert np.array_equal(m_g, oracle.mask(u_c))
        for k in range(3):
            assert c1g[k] == pytest.approx(oracle.region_mean(planes[k], u_c, 0), rel=1e-9)
            assert c2g[k] == pytest.approx(oracle.region_mean(planes[k], u_c, 1), rel=1e-9)


def test_resident_c3_chunks_continuation_and_mixing(capi, oracle):
    """Chunk boundaries (enqueue 5 + 8 + 1), a second run from the result, then the per-launch flow from the resident result and
    back: all equal the oracle's 30 iterations; the flow is bitwise repeatable."""
    h, w = 160, 384
    planes = colour_disk(h, w, noise=12, seed=9)
    u0 = oracle.checkerboard(h, w)
    pk = dict(tol=0, **LAM)
    u_c, _, _, tr_c = oracle.csv_run(planes, u0, oracle.make_params(**pk), 30)
    outs = []
    for rep in range(2):
        ctx, _ = resident_ctx(capi, h, w, pk)
        with ctx:
            ctx.set_option("trace", 64)
            ctx.set_image(planes)
            ctx.set_levelset(u0)
            ctx.enqueue_steps(5); ctx.enqueue_steps(8); ctx.enqueue_steps(1)
            done, _, stopped = ctx.sync()
            assert done == 14 and not stopped
            tr = ctx.get_trace(14)
            assert tr.shape == (14, 7) and np.allclose(tr, tr_c[:14], rtol=1e-9, atol=0)
            assert ctx.run(6)[0] == 6                     # resident, continues from the level set in memory
            ctx.set_option("resident", 0)
            assert ctx.launch_info()["kernel"].startswith("csv_wave")
            assert ctx.run(7)[0] == 7                     # per-launch flow from the resident result
            ctx.set_option("resident", 1)
            assert ctx.launch_info()["kernel"].startswith("csv_resident_kernel<3")
            assert ctx.run(3)[0] == 3                     # and back
            outs.append(ctx.get_levelset())
    print("c3 mixing rel_err", rel_err(outs[0], u_c))
    assert rel_err(outs[0], u_c) <= 1e-9
    assert np.array_equal(outs[0], outs[1])


def test_resident_c3_stop_rule_same_iteration(capi, oracle):
    """The stop rule is booked at the grid barrier of the iteration itself: the run ends at the reference's iteration (first chunk,
    middle of a chunk), and the level set is the reference's (test_resident_stop_rule_same_iteration's bounds)."""
    planes = colour_disk(128, 128, noise=0)
    u0 = oracle.checkerboard(128, 128)
    for tol in (1e-3, 0.05, 0.5):
        u_c, done_c, nrm_c, _ = oracle.csv_run(planes, u0, oracle.make_params(tol=tol), 400)
        for sync_every in (1, 7, 32):
            ctx, _ = resident_ctx(capi, 128, 128, dict(tol=tol))
            with ctx:
                ctx.set_option("sync_every", sync_every)
                ctx.set_image(planes)
                ctx.set_levelset(u0)
                done_g, nrm_g = ctx.run(400)
                u_g = ctx.get_levelset()
            assert done_g == done_c, (tol, sync_every, done_g, done_c)
            assert nrm_g == pytest.approx(nrm_c, rel=1e-7)
            assert rel_err(u_g, u_c) <= 1e-6


LARGE = [(1080, 1920), (1536, 2048)]      # 17 x 15 tiles of 63 / 64 rows; the largest plane: 16 x 16 tiles of 96 rows


@pytest.mark.parametrize("shape", LARGE)
def test_resident_c3_against_the_per_launch_flow_at_scale(capi, shape):
    """One context, 60 iterations from the checkerboard on the noisy colour disk, in both flows: <= 1e-9 (the two flows agree to 1e-9,
    not bit for bit: DESIGN.md 6)."""
    h, w = shape
    planes = colour_disk(h, w, noise=20, seed=31)
    pk = dict(tol=0, nu=0.01, **LAM)
    steps = 60
    ctx, info = resident_ctx(capi, h, w, pk)
    with ctx:
        ctx.set_option("trace", steps)
        ctx.set_image(planes); ctx.init_checkerboard()
        assert ctx.run(steps)[0] == steps
        u_r, tr_r, m_r = ctx.get_levelset(), ctx.get_trace(steps), ctx.get_mask()
        ctx.set_option("resident", 0)
        assert ctx.launch_info()["kernel"].startswith("csv_wave")
        ctx.init_checkerboard()
        assert ctx.run(steps)[0] == steps
        u_l, tr_l, m_l = ctx.get_levelset(), ctx.get_trace(steps), ctx.get_mask()
    print("c3 scale", shape, info["tiles_y"], info["tiles_x"], "rel_err", rel_err(u_r, u_l), "trace", float(np.abs(tr_r / tr_l - 1).max()))
    assert tr_r.shape == (steps, 7)
    assert rel_err(u_r, u_l) <= 1e-9, rel_err(u_r, u_l)
    assert np.allclose(tr_r, tr_l, rtol=1e-9, atol=0)
    assert np.array_equal(m_r, m_l)


def test_resident_c3_chunking_does_not_change_bits(capi):
    h, w = 1080, 1920
    planes = colour_disk(h, w, noise=20, seed=31)
    outs = []
    for chunk in (1, 7, 42):
        ctx, _ = resident_ctx(capi, h, w, dict(tol=0, nu=0.01, **LAM))
        with ctx:
            ctx.set_option("trace", 42)
            ctx.set_image(planes); ctx.init_checkerboard()
            for _ in range(42 // chunk):
                ctx.enqueue_steps(chunk)
            assert ctx.sync()[0] == 42
            outs.append((ctx.get_levelset(), ctx.get_trace(42)))
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])


@pytest.mark.parametrize("shape,flavour", [((16, 128), 2), ((64, 256), 2), ((512, 512), 2), ((1024, 1024), 4), ((1024, 2048), 8)])
def test_resident_c3_straight_line_flavours_are_the_generic_march_bit_for_bit(capi, shape, flavour):
    """Tiles of exactly 16 / 32 / 64 rows run csv_resident_kernel<3, 2 | 4 | 8> (a 96-row tile is 12 rows per wave: the generic march; 128
    rows do not fit with three channels): level set and trace are those of the generic flavour ("res_straight" = 0) bit for bit."""
    h, w = shape
    planes = colour_disk(h, w, noise=30, seed=5)
    outs = []
    for straight in (1, 0):
        with capi.Context(h, w, 3, capi.make_params(tol=0, nu=0.01, **LAM)) as ctx:
            ctx.set_option("resident", 1); ctx.set_option("res_straight", straight); ctx.set_option("trace", 25)
            assert ctx.launch_info()["kernel"] == "csv_resident_kernel<3, %d>" % (flavour if straight else 0)
            ctx.set_image(planes); ctx.init_checkerboard()
            assert ctx.run(25)[0] == 25
            outs.append((ctx.get_levelset(), ctx.get_trace(25)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("shape", [(384, 640), (1536, 2048)])
def test_resident_c3_release_lines_shared_or_not_same_results(capi, shape):
    """Which release line a tile polls ("res_go_share": 5 a line per XCD, 0 a line per tile) is plumbing: the same bits, with a chunk
    boundary in the middle -- 15 and 256 tiles."""
    h, w = shape
    planes = colour_disk(h, w, noise=20, seed=11)
    outs = []
    for share in (5, 0):
        ctx, _ = resident_ctx(capi, h, w, dict(tol=0, nu=0.01, **LAM))
        with ctx:
            ctx.set_option("res_go_share", share); ctx.set_option("trace", 40)
            ctx.set_image(planes); ctx.init_checkerboard()
            ctx.enqueue_steps(9); ctx.enqueue_steps(14); ctx.sync()
            outs.append((ctx.get_levelset(), ctx.get_trace(23)))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("near_switch", [1, 0])
def test_resident_c3_near_regime(capi, oracle, near_switch):
    """dt = 0.001: every pixel stays below the far-field threshold of H_eps for the whole run -- the table form on every lane
    ("near_switch" = 1) or the far form with the per-group correction (0): each <= 1e-9 against the oracle."""
    h, w = 200, 384
    planes = colour_disk(h, w, noise=12, seed=3)
    u0 = oracle.checkerboard(h, w)
    pk = dict(tol=0, dt=0.001, **LAM)
    u_c, _, nrm_c, tr_c = oracle.csv_run(planes, u0, oracle.make_params(**pk), 20)
    assert np.abs(u_c).max() < 32.0                        # below 32 eps everywhere
    ctx, _ = resident_ctx(capi, h, w, pk)
    with ctx:
        ctx.set_option("near_switch", near_switch); ctx.set_option("trace", 20)
        ctx.set_image(planes); ctx.set_levelset(u0)
        done, nrm = ctx.run(20)
        u_g, tr_g = ctx.get_levelset(), ctx.get_trace(20)
    print("c3 near", near_switch, "rel_err", rel_err(u_g, u_c))
    assert done == 20
    assert rel_err(u_g, u_c) <= 1e-9, rel_err(u_g, u_c)
    assert np.allclose(tr_g, tr_c, rtol=1e-9, atol=0)
    assert nrm == pytest.approx(nrm_c, rel=1e-9)


@pytest.mark.parametrize("shape", [(1537, 2048), (64, 130 + 1)])
def test_a_plane_that_does_not_qualify_keeps_the_per_launch_flow(capi, oracle, shape):
    """One row more than 256 tiles of 96 rows hold, or an odd width: "resident" = 1 silently keeps the per-launch flow."""
    h, w = shape
    planes = colour_disk(h, w, noise=10, seed=2)
    u0 = oracle.checkerboard(h, w)
    pk = dict(tol=0, **LAM)
    u_c, _, _, _ = oracle.csv_run(planes, u0, oracle.make_params(**pk), 5)
    with capi.Context(h, w, 3, capi.make_params(**pk)) as ctx:
        ctx.set_option("resident", 1)
        assert ctx.launch_info()["kernel"].startswith("csv_wave"), ctx.launch_info()
        ctx.set_image(planes); ctx.set_levelset(u0)
        assert ctx.run(5)[0] == 5
        assert rel_err(ctx.get_levelset(), u_c) <= 1e-9


def test_automatic_is_unchanged_for_three_channels(capi):
    with capi.Context(512, 512, 3) as ctx:
        assert ctx.launch_info()["kernel"].startswith("csv_wave"), ctx.launch_info()
        ctx.set_option("resident", 1)
        assert ctx.launch_info()["kernel"] == "csv_resident_kernel<3, 2>"
        ctx.set_option("resident", -1)
        assert ctx.launch_info()["kernel"].startswith("csv_wave")
