"""Perona-Malik batch (cvh_perona_malik_batch): the planes of several contexts share cooperative launches of the resident kernel.  Every
member's uint8 planes must be BYTE-IDENTICAL to the same image smoothed by its own cvh_perona_malik on a fresh context, whatever the
batch mixes (shapes, K / L / T, FAST / STRICT, 1 / 3 channels, member order, members that take their own flow); STRICT members equal
the oracle, FAST ones meet test_gpu_pm_resident.py's bar."""
import ctypes as C

import numpy as np
import pytest

from chan_vese_amd import synth

pytestmark = pytest.mark.gpu

STRICT, FAST = 1, 2
ERR_ARG, ERR_STATE = 1, 3


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    return m


def rand_planes(h, w, ch, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w), dtype=np.uint8) for _ in range(ch)]


def make(capi, planes, math, **opts):
    h, w = planes[0].shape
    ctx = capi.Context(h, w, len(planes))
    ctx.set_option("math_mode", math)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_image(planes)
    return ctx


def own(capi, planes, math, K, L, T, **opts):
    with make(capi, planes, math, **opts) as ctx:
        ctx.perona_malik(K, L, T)
        return ctx.get_image()


def num_cus(capi, ctx):
    out = C.c_int(0)
    fn = capi.lib().cvh_debug_num_cus
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    assert fn(ctx._h, C.byref(out)) == 0
    return out.value


def assert_oracle(oracle, planes, gpu, K, L, T, math):
    for g, c in zip(gpu, oracle.perona_malik(planes, K, L, T)):
        if math == STRICT:
            assert np.array_equal(g, c)
        else:
            d = np.abs(g.astype(int) - c.astype(int))
            assert d.max() <= 1 and (d != 0).sum() <= max(1, int(1e-6 * d.size))


# (shape, channels, math, K, L, T): one tile, ragged last tile column, short last tile row, 600 x 132, distinct K / L / T per member
# (so step counts differ inside one launch), both flavours, 1 and 3 channels
MIXED = [((16, 16), 1, FAST, 30, 0.25, 5.0),
         ((37, 130), 3, STRICT, 10, 0.2, 3.0),
         ((70, 372), 1, STRICT, 1000, 0.1, 1.5),
         ((600, 132), 3, FAST, 20, 0.25, 10.0),
         ((333, 260), 1, FAST, 30, 0.15, 6.0),
         ((128, 128), 1, STRICT, 5, 0.25, 2.0),
         ((130, 256), 3, FAST, 12, 0.05, 0.75)]


def test_mixed_members_are_byte_identical_to_their_own_runs_and_meet_the_oracle(capi, oracle):
    planes = [rand_planes(s[0], s[1], ch, 11 + i) for i, (s, ch, *_) in enumerate(MIXED)]
    refs = [own(capi, p, m, K, L, T) for p, (_, _, m, K, L, T) in zip(planes, MIXED)]
    for i, (p, (_, _, m, K, L, T)) in enumerate(zip(planes, MIXED)):
        assert_oracle(oracle, p, refs[i], K, L, T, m)
    for order in (list(range(len(MIXED))), list(reversed(range(len(MIXED))))):
        ctxs = [make(capi, planes[i], MIXED[i][2]) for i in order]
        capi.perona_malik_batch(ctxs, [MIXED[i][3] for i in order], [MIXED[i][4] for i in order], [MIXED[i][5] for i in order])
        for ctx, i in zip(ctxs, order):
            got = ctx.get_image()
            for g, r in zip(got, refs[i]):
                assert np.array_equal(g, r), (order, i)
            info = ctx.launch_info(1)
            want = "pm_resident_batch_kernel<%s, " % ("true" if MIXED[i][2] == FAST else "false")
            assert info["kernel"].startswith(want), info
            assert int(info["trips"]) == oracle.pm_trip_count(MIXED[i][4], MIXED[i][5])
            assert int(info["batch_planes"]) >= 1 and int(info["batch_launches"]) >= 1
            assert ctx.last_pm_ms() > 0
            ctx.close()


def test_more_tiles_than_one_launch_holds(capi):
    """70 x 256^2: 280 tiles of 128^2 at the longest band, more than the CUs hold at once -> two or more launches."""
    n, K, L, T = 70, 30, 0.25, 2.0
    imgs = [synth.disk(256, 200, 50, noise=30, seed=100 + b, radius=50 + b % 20) for b in range(n)]
    ctxs = [make(capi, [img], FAST) for img in imgs]
    cus = num_cus(capi, ctxs[0])
    capi.perona_malik_batch(ctxs, K, L, T)
    infos = [ctx.launch_info(1) for ctx in ctxs]
    if 4 * n > min(cus, 256):
        assert int(infos[0]["batch_launches"]) >= 2, infos[0]
    assert 4 * int(infos[0]["batch_planes"]) <= min(cus, 256) and int(infos[0]["tiles_y"]) * int(infos[0]["tiles_x"]) == 4
    for ctx, img in zip(ctxs, imgs):
        assert np.array_equal(ctx.get_image()[0], own(capi, [img], FAST, K, L, T)[0])
        ctx.close()


def test_a_large_member_beside_small_ones_and_members_that_take_their_own_flow(capi):
    K, L, T = 25, 0.25, 2.0
    members = [(rand_planes(2048, 2048, 1, 1), FAST, {}),
               (rand_planes(256, 256, 1, 2), FAST, {}),
               (rand_planes(40, 57, 1, 3), FAST, {}),                        # odd width: the per-launch flow
               (rand_planes(200, 256, 3, 4), STRICT, {}),
               (rand_planes(256, 256, 1, 5), FAST, {"pm_kernel": 3}),         # the 2-step per-launch kernel, chosen
               (rand_planes(128, 384, 1, 6), STRICT, {"pm_strip_rows": 16}),  # tuned per-launch geometry
               (rand_planes(96, 96, 1, 7), STRICT, {"pm_kernel": 4})]         # the resident kernel, chosen: fused
    ctxs = [make(capi, p, m, **o) for p, m, o in members]
    big = num_cus(capi, ctxs[0]) >= 256          # a 2048^2 plane is 256 tiles of 128^2: resident where the device holds them
    capi.perona_malik_batch(ctxs, K, L, T)
    for i, (ctx, (p, m, o)) in enumerate(zip(ctxs, members)):
        got = ctx.get_image()
        ref = own(capi, p, m, K, L, T, **o)
        for g, r in zip(got, ref):
            assert np.array_equal(g, r), i
        kernel = ctx.launch_info(1)["kernel"]
        assert kernel.startswith("pm_resident_batch_kernel") == (i in (1, 3, 6) or (i == 0 and big)), (i, kernel)
        ctx.close()


def test_pm_batch_then_run_batch_matches_own_runs_and_the_oracle(capi, oracle):
    """The whole pipeline, batched: Perona-Malik, then cvh_run_batch.  STRICT members, whose smoothed planes are the oracle's bytes, so
    that the oracle's Perona-Malik-then-CSV starts from the very planes the batch produced (a FAST plane may differ by 1 LSB in a pixel,
    which moves the level set far more than 1e-9).  The oracle bar of the fused-batch tests, 1e-9 of max|u|, after 8 iterations; after
    all 70 (the level set grows to ~2000 from the checkerboard) every CSV flow, batched or not, drifts to ~3e-9 of it: 1e-8 there, with
    the masks' overlap."""
    K, L, T, steps = 30, 0.25, 3.0, 70
    shapes = [(256, 256)] * 6 + [(512, 512)] * 2
    imgs = [synth.disk(h, 200, 50, noise=20, seed=40 + b, radius=h // 4 + 3 * b) for b, (h, w) in enumerate(shapes)]
    params = capi.make_params(tol=1e-3)
    ctxs = []
    for img in imgs:
        ctx = capi.Context(img.shape[0], img.shape[1], 1, params)
        ctx.set_option("math_mode", STRICT)
        ctx.set_image([img])
        ctxs.append(ctx)
    capi.perona_malik_batch(ctxs, K, L, T)
    pms = []
    for ctx, img in zip(ctxs, imgs):
        pm = oracle.perona_malik([img], K, L, T)
        assert np.array_equal(ctx.get_image()[0], pm[0])
        pms.append(pm)
    for n, bar in ((8, 1e-9), (steps, 1e-8)):
        for ctx in ctxs:
            ctx.init_checkerboard()
        res = capi.run_batch(ctxs, n)
        for ctx, pm, (done, nrm) in zip(ctxs, pms, res):
            h, w = pm[0].shape
            u_cpu, done_cpu, _, _ = oracle.csv_run(pm, oracle.checkerboard(h, w), oracle.make_params(tol=1e-3), n, trace=False)
            assert done == done_cpu
            u = ctx.get_levelset()
            assert np.abs(u - u_cpu).max() <= bar * np.abs(u_cpu).max(), (h, w, n, np.abs(u - u_cpu).max() / np.abs(u_cpu).max())
            if n == steps:
                m, mc = ctx.get_mask().astype(bool), oracle.mask(u_cpu).astype(bool)
                assert (m & mc).sum() / max((m | mc).sum(), 1) >= 0.999
    for ctx, img, (done, nrm) in zip(ctxs, imgs, res):
        h, w = img.shape
        with capi.Context(h, w, 1, params) as ref:
            ref.set_option("math_mode", STRICT)
            ref.set_image([img])
            ref.perona_malik(K, L, T)
            assert np.array_equal(ctx.get_image()[0], ref.get_image()[0])
            ref.init_checkerboard()
            ref_done, _ = ref.run(steps)
            assert ctx.get_stop_condition() == ref.get_stop_condition()
            assert done == ref_done
        ctx.close()


def test_refusals_leave_every_member_untouched(capi):
    L_ = capi.lib()
    planes = [rand_planes(64, 64, 1, 20 + i) for i in range(4)]
    ctxs = [make(capi, p, FAST) for p in planes]
    with pytest.raises(capi.CvhError) as e:
        capi.perona_malik_batch(ctxs, 30, [0.25, 0.25, 0.3, 0.25], 1.0)
    assert e.value.code == ERR_ARG and "member 2" in str(e.value)
    assert b"member 2" in L_.cvh_last_error(None)
    for ctx, p in zip(ctxs, planes):
        assert np.array_equal(ctx.get_image()[0], p[0])
    with pytest.raises(capi.CvhError) as e:
        capi.perona_malik_batch([ctxs[0], ctxs[1], ctxs[0]], 30, 0.25, 1.0)   # a duplicate
    assert e.value.code == ERR_ARG and "member 2" in str(e.value)
    with pytest.raises(capi.CvhError) as e:
        capi.perona_malik_batch(ctxs, 30, 0.25, [1.0, 0.1, 1.0, 1.0])        # T < L
    assert e.value.code == ERR_ARG and "member 1" in str(e.value)
    with pytest.raises(capi.CvhError) as e:
        capi.perona_malik_batch(ctxs, [30, 30, 30, 0], 0.25, 1.0)             # K = 0
    assert e.value.code == ERR_ARG and "member 3" in str(e.value)
    with capi.Context(64, 64, 1) as bare:                                      # no image
        with pytest.raises(capi.CvhError) as e:
            capi.perona_malik_batch([ctxs[0], bare], 30, 0.25, 1.0)
        assert e.value.code == ERR_STATE and "member 1" in str(e.value)
    with make(capi, rand_planes(40, 57, 1, 9), FAST, pm_kernel=4) as odd:     # pm_kernel 4 on a plane that does not qualify
        with pytest.raises(capi.CvhError) as e:
            capi.perona_malik_batch([ctxs[0], odd], 30, 0.25, 1.0)
        assert e.value.code == ERR_ARG and "member 1" in str(e.value)
    for ctx, p in zip(ctxs, planes):
        assert np.array_equal(ctx.get_image()[0], p[0])
        ctx.close()


def test_unsynchronised_csv_work_is_closed_first(capi):
    """A member with CSV iterations enqueued and not synchronised ends with the planes and the level set it has when it is synced first."""
    img, other = rand_planes(256, 256, 1, 31), rand_planes(128, 256, 1, 32)
    out = []
    for sync_first in (False, True):
        a, b = make(capi, img, FAST), make(capi, other, FAST)
        a.init_checkerboard()
        a.enqueue_steps(5)
        if sync_first:
            a.sync()
        capi.perona_malik_batch([b, a], 30, 0.25, 4.0)
        out.append((a.get_image()[0], a.get_levelset(), b.get_image()[0]))
        a.close()
        b.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][2], out[1][2])
    assert out[0][1].tobytes() == out[1][1].tobytes()
