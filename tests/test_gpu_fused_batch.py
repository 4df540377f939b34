"""Fused batch (cvh_run_batch / cvh_enqueue_steps_batch): N contexts advance with one launch per iteration and CSV-step
instantiation.  Every member computes the same bits as its own per-launch run on the same strips (level set, every trace
row, steps_done, stopped), stops at its own iteration, matches the oracle with automatic geometry, continues its own runs
(resident flow included) without a sync in between, and the argument errors leave the members usable."""
import numpy as np
import pytest

from chan_vese_amd import synth
from fused_batch_util import STRICT, assert_same, cone, iou, member, planes, result, tol_for_stop

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def test_fused_bits_equal_own_runs(capi):
    specs = [(512, 512, 1, {}), (480, 640, 1, {}), (278, 370, 1, {"math_mode": STRICT}), (1024, 1024, 3, {}),
             (1080, 1920, 1, {}), (1080, 1920, 1, {})]
    ctxs = [member(capi, h, w, ch, dict(opts, strip_rows=16, resident=0), seed=10 + i) for i, (h, w, ch, opts) in enumerate(specs)]
    kernels = [c.launch_info()["kernel"] for c in ctxs]
    assert kernels[1].startswith("csv_wave_kernel<") and kernels[2].startswith("csv_wave_kernel<1, false")   # kernel 2, FAST and STRICT
    assert kernels[3].startswith("csv_wave2_kernel<3") and kernels[4].startswith("csv_wave2_kernel<1")
    steps = 40
    for c in ctxs:
        c.init_checkerboard()
    out = capi.run_batch(ctxs, steps)
    fused = [result(c, steps) for c in ctxs]
    assert [d for d, _ in out] == [steps] * len(ctxs)
    for c in ctxs:
        c.init_checkerboard()
        assert c.run(steps)[0] == steps
    own = [result(c, steps) for c in ctxs]
    for i in range(len(ctxs)):
        assert_same(fused[i], own[i], (i, specs[i], kernels[i]))
        assert out[i][1] == own[i][1][steps - 1, -1]
    for c in ctxs:
        c.close()


def test_fused_members_stop_at_their_own_iteration(capi):
    """tol per member such that one stops inside the first poll chunk (sync_every = 32), two later; the fourth never stops."""
    pk = dict(nu=0.01, dt=0.5)
    specs = [((512, 512, 1), 12), ((480, 640, 1), 45), ((1024, 1024, 1), 70), ((256, 384, 3), 0)]
    ctxs = [member(capi, h, w, ch, dict(strip_rows=16, resident=0), seed=20 + i, trace=128, **pk) for i, ((h, w, ch), _) in enumerate(specs)]
    for c, (_, k) in zip(ctxs, specs):
        c.set_params(capi.make_params(tol=tol_for_stop(capi, c, k, 90, pk) if k else 0.0, **pk))
    steps = 100
    for c in ctxs:
        c.set_levelset(cone(c.h, c.w))
    out = capi.run_batch(ctxs, steps)
    fused = [result(c, 128) for c in ctxs]
    assert [d for d, _ in out] == [k or steps for _, k in specs]
    for c in ctxs:
        c.set_levelset(cone(c.h, c.w))
        c.run(steps)
    own = [result(c, 128) for c in ctxs]
    for i, (spec, k) in enumerate(specs):
        assert fused[i][2] == (k or steps) and fused[i][3] == bool(k), (spec, fused[i][2:])
        assert_same(fused[i], own[i], spec)
    for c in ctxs:
        c.close()


def test_fused_against_oracle(capi, oracle):
    """Automatic geometry (each member's strips sized for its share of the chip): the bar of test_resident_small_shapes."""
    pk = dict(tol=0, nu=0.01, dt=0.5)
    shapes = [(512, 512, 1), (256, 384, 3)]
    ctxs = [member(capi, h, w, ch, seed=30 + i, trace=128, **pk) for i, (h, w, ch) in enumerate(shapes)]
    imgs = [planes(h, w, ch, 30 + i) for i, (h, w, ch) in enumerate(shapes)]
    u0 = [oracle.checkerboard(h, w) for h, w, _ in shapes]
    for steps in (1, 2, 9):
        for c, u in zip(ctxs, u0):
            c.set_levelset(u)
        out = capi.run_batch(ctxs, steps)
        for i, c in enumerate(ctxs):
            u_c, done_c, nrm_c, tr_c = oracle.csv_run(imgs[i], u0[i], oracle.make_params(**pk), steps)
            u_g = c.get_levelset()
            assert out[i][0] == done_c == steps
            assert np.abs(u_g - u_c).max() / np.abs(u_c).max() <= 1e-9, (shapes[i], steps)
            assert np.allclose(c.get_trace(steps), tr_c, rtol=1e-9, atol=0), (shapes[i], steps)
            assert np.array_equal(c.get_mask(), oracle.mask(u_c)), (shapes[i], steps)
    for c, u in zip(ctxs, u0):
        c.set_levelset(u)
    capi.run_batch(ctxs, 100)
    for i, c in enumerate(ctxs):
        u_c = oracle.csv_run(imgs[i], u0[i], oracle.make_params(**pk), 100)[0]
        assert iou(c.get_mask().astype(bool), oracle.mask(u_c).astype(bool)) >= 0.999, shapes[i]
    for c in ctxs:
        c.close()


def continuation(capi, main, others, sync_between):
    main.set_levelset(cone(main.h, main.w))
    main.reset_run()
    for o in others:
        o.init_checkerboard()
        o.reset_run()

    def settle(ctxs):
        if sync_between:
            for c in ctxs:
                c.sync()

    main.enqueue_steps(10)                                   # its own run: the resident kernel
    settle([main])
    capi.enqueue_steps_batch([others[0], main] + others[1:], 20)   # main is not the leader: its stream joins another's
    settle([main] + others)
    main.enqueue_steps(10)
    settle([main])
    for o in others:
        o.sync()
    return result(main, 40)


def test_fused_continuation_with_own_runs(capi):
    main = member(capi, 1024, 1024, seed=40, opts={"resident": 1})
    assert main.launch_info()["kernel"].startswith("csv_resident_kernel<")
    others = [member(capi, 512, 512, seed=41 + i) for i in range(3)]
    ref = continuation(capi, main, others, True)
    assert ref[2] == 40 and not ref[3]
    got = continuation(capi, main, others, False)
    assert_same(got, ref, "tol = 0")
    # tol from the reference run's norms: the stop falls on iteration 30, the last fused one
    norms = ref[1][:, -1]
    main.set_params(capi.make_params(tol=1.0))
    scale = main.get_stop_condition()
    assert norms[:29].min() > norms[29] * (1 + 1e-5)
    main.set_params(capi.make_params(tol=norms[29] / scale * (1 + 1e-6)))
    ref = continuation(capi, main, others, True)
    got = continuation(capi, main, others, False)
    assert ref[2] == 30 and ref[3], ref[2:]
    assert got[2] == 30 and got[3], got[2:]
    assert_same(got, ref, "stop at 30")
    for c in [main] + others:
        c.close()


def test_fused_errors_leave_members_usable(capi):
    a, b = member(capi, 256, 256, seed=50), member(capi, 256, 384, seed=51)
    for c in (a, b):
        c.init_checkerboard()
    with pytest.raises(capi.CvhError) as e:
        capi.run_batch([a, b, a], 5)
    assert e.value.code == 1 and "member 2 duplicates member 0" in str(e.value)
    b.set_option("finalize", 1)
    with pytest.raises(capi.CvhError) as e:
        capi.enqueue_steps_batch([a, b], 5)
    assert e.value.code == 1 and "member 1" in str(e.value) and "finalize" in str(e.value)
    b.set_option("finalize", 0)
    bare = capi.Context(128, 128)
    bare.set_image(planes(128, 128, 1, 52))
    with pytest.raises(capi.CvhError) as e:
        capi.run_batch([a, b, bare], 5)
    assert e.value.code == 3 and "member 2" in str(e.value) and "level set" in str(e.value)
    with pytest.raises(capi.CvhError) as e:
        capi.run_batch([], 5)
    assert e.value.code == 1
    assert [d for d, _ in capi.run_batch([a, b], 5)] == [5, 5]
    assert a.run(3)[0] == 3 and b.run(3)[0] == 3
    for c in (a, b, bare):
        c.close()


def test_fused_scale_64_members(capi):
    n, steps = 256, 200
    radii = [n // 4 + 4 * (k % 8) - 16 for k in range(64)]
    ctxs = []
    for k in range(64):
        c = capi.Context(n, n, 1, capi.make_params(tol=0.0))
        c.set_option("strip_rows", 16)
        c.set_image([synth.disk(n, 200, 50, noise=16, seed=500 + k, radius=radii[k])])
        c.init_checkerboard()
        ctxs.append(c)
    out = capi.run_batch(ctxs, steps)
    assert [d for d, _ in out] == [steps] * 64
    ii = np.arange(n)[:, None] - n // 2
    jj = np.arange(n)[None, :] - n // 2
    u17 = None
    for k, c in enumerate(ctxs):
        # From a checkerboard start the sign of the converged level set is not fixed by the image (both occur in this batch), so the
        # mask (u > 0) must be the disk exactly where the member's own region mean c1 (of H(u) ~ u > 0) is the disk's level, 200.
        m = c.get_mask().astype(bool)
        d = ii * ii + jj * jj <= radii[k] * radii[k]
        c1, c2 = c.get_means()
        mask_is_disk = abs(c1[0] - 200) < 5 and abs(c2[0] - 50) < 5
        assert mask_is_disk or (abs(c1[0] - 50) < 5 and abs(c2[0] - 200) < 5), (k, c1, c2)
        assert iou(m, d if mask_is_disk else ~d) >= 0.999, (k, mask_is_disk)
        assert iou(c.get_mask(invert=True).astype(bool), ~d if mask_is_disk else d) >= 0.999, k
        if k == 17:
            u17 = c.get_levelset().tobytes()
    ctxs[17].init_checkerboard()
    assert ctxs[17].run(steps)[0] == steps
    assert ctxs[17].get_levelset().tobytes() == u17
    for c in ctxs:
        c.close()
