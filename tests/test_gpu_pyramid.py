"""Coarse-to-fine on the GPU (cvh_restrict_image*, cvh_prolong_levelset*, capi.run_coarse_to_fine*) against the numpy restatement of the
header's definitions (pyramid_util).  Restrict is defined in integers and prolong is a bit copy, so every comparison of planes, level sets,
traces and stop conditions is == (on bit patterns for doubles); only the run against the CPU oracle has bars, and they are the issue's:
per-level step counts within +-2, finest mask IoU >= 0.999.  Not covered here: the two CVH_ERR_ARG cases that no quick test can build --
pairs on different devices (needs two GPUs; checked where there are two) and a fine plane of 2^32 pixels (tens of GB of level set).
Run with -m gpu on an MI355X."""
import ctypes

import numpy as np
import pytest

import pyramid_util as U

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = 1, 3


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def alone(ctx, **opts):
    """contexts compared in bits must not see each other in their automatic choices (tests/test_gpu_device_io.py, same_choices)"""
    ctx.set_option("co_resident", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def same_run(a, b, steps=5):
    """a and b hold the same image and level set: means, a traced run and the level set behind it agree in bits"""
    for x, y in zip(a.get_means(), b.get_means()):
        assert np.array_equal(U.bits(x), U.bits(y))
    ra, rb = a.run(steps), b.run(steps)
    assert ra[0] == rb[0] and U.bits(np.float64(ra[1])) == U.bits(np.float64(rb[1]))
    assert np.array_equal(U.bits(a.get_trace(steps)), U.bits(b.get_trace(steps)))
    assert np.array_equal(U.bits(a.get_levelset()), U.bits(b.get_levelset()))


def launches():
    fn = ctypes.CDLL(__import__("chan_vese_amd").capi.LIB_PATH).cvh_debug_pyramid_launches
    fn.restype = ctypes.c_ulong
    return fn()


ids = dict(ids=lambda s: f"{s[0]}x{s[1]}")


@pytest.mark.parametrize("channels", U.CHANNELS)
@pytest.mark.parametrize("shape", U.SHAPES, **ids)
def test_restrict(capi, shape, channels):
    h, w = shape
    hc, wc = U.coarse_shape(h, w)
    p = capi.make_params(tol=2.0 ** -40)   # (a power of two: equal stop conditions are equal norms, and no run of five iterations stops)
    with capi.Context(h, w, channels, p) as fine, capi.Context(h, w, channels, p) as fine2, capi.Context(hc, wc, channels, p) as coarse, \
            capi.Context(hc, wc, channels, p) as control:
        for c in (fine, fine2, coarse, control):
            alone(c, trace=8)
        u0 = U.smooth_levelset(hc, wc)
        coarse.set_levelset(u0)                       # before the planes arrive: restrict treats it as cvh_set_image does
        for kind in ("all255", "all0", "random"):
            planes = U.planes_of(kind, h, w, channels)
            want = [U.restrict(q) for q in planes]
            fine.set_image(planes)
            fine.restrict_image_to(coarse)
            assert all(np.array_equal(a, b) for a, b in zip(coarse.get_image(), want)), kind
            control.set_image(want)
            control.set_levelset(u0)
            assert coarse.get_stop_condition() == control.get_stop_condition(), kind
            assert np.array_equal(U.bits(coarse.get_levelset()), U.bits(u0))
            if kind == "all255":
                assert all((q == 255).all() for q in want)     # no overflow, rounding at the top
        same_run(coarse, control)
        # the fine context is only read, its iterations stay in flight across the call
        fine2.set_image(planes)
        uf = U.smooth_levelset(h, w)
        for c in (fine, fine2):
            c.set_levelset(uf)
            c.enqueue_steps(3)
        fine.restrict_image_to(coarse)
        for c in (fine, fine2):
            c.enqueue_steps(2)
        sa, sb = fine.sync(), fine2.sync()
        assert sa[0] == sb[0] == 5 and U.bits(np.float64(sa[1])) == U.bits(np.float64(sb[1]))
        assert np.array_equal(U.bits(fine.get_levelset()), U.bits(fine2.get_levelset()))
        assert all(np.array_equal(a, b) for a, b in zip(fine.get_image(), planes))
        assert all(np.array_equal(a, b) for a, b in zip(coarse.get_image(), want))
        # after Perona-Malik the smoothed planes are what is averaged
        fine.perona_malik(K=10.0, L=0.25, T=1.0)
        smoothed = fine.get_image()
        assert any(not np.array_equal(a, b) for a, b in zip(smoothed, planes))
        fine.restrict_image_to(coarse)
        assert all(np.array_equal(a, U.restrict(b)) for a, b in zip(coarse.get_image(), smoothed))


@pytest.mark.parametrize("shape", U.SHAPES, **ids)
def test_prolong(capi, shape):
    h, w = shape
    hc, wc = U.coarse_shape(h, w)
    p = capi.make_params(tol=0.0)
    with capi.Context(hc, wc, 1, p) as coarse, capi.Context(h, w, 1, p) as fine, capi.Context(h, w, 1, p) as control:
        for c in (coarse, fine, control):
            alone(c, trace=8)
        planes = U.planes_of("random", h, w, 1)
        fine.set_image(planes)
        control.set_image(planes)
        fine.set_levelset(np.ones((h, w)))
        fine.run(2)                                    # a run the new level set ends
        uc = U.special_levelset(hc, wc)
        coarse.set_levelset(uc)
        coarse.prolong_levelset_to(fine)
        assert np.array_equal(U.bits(fine.get_levelset()), U.bits(U.prolong(uc, h, w)))
        assert np.array_equal(U.bits(U.prolong(uc, h, w))[::2, ::2], U.bits(uc))
        assert np.array_equal(fine.get_mask(), U.prolong_mask(coarse.get_mask(), h, w))
        assert fine.sync()[0] == 0                      # a new run
        assert np.array_equal(U.bits(coarse.get_levelset()), U.bits(uc))
        # an ordinary level set (the special one is NaN after one iteration), then five iterations like cvh_set_levelset's
        uc = U.smooth_levelset(hc, wc)
        coarse.set_levelset(uc)
        coarse.prolong_levelset_to(fine)
        control.set_levelset(U.prolong(uc, h, w))
        assert np.array_equal(U.bits(fine.get_levelset()), U.bits(control.get_levelset()))
        same_run(fine, control)


def test_prolong_into_and_out_of_float_state(capi):
    p = capi.make_params(tol=0.0)
    # coarse 64 -> fine 32 at (32, 160): the fine float pair adopts the level set, as after cvh_set_levelset
    with capi.Context(16, 80, 1, p) as coarse, capi.Context(32, 160, 1, p) as fine, capi.Context(32, 160, 1, p) as control:
        planes = U.planes_of("random", 32, 160, 1)
        for c in (fine, control):
            alone(c, state=32, trace=8)
            c.set_image(planes)
        uc = U.smooth_levelset(16, 80) * 1.0000001   # (not floats)
        coarse.set_levelset(uc)
        coarse.prolong_levelset_to(fine)
        control.set_levelset(U.prolong(uc, 32, 160))
        got = fine.get_levelset()
        assert np.array_equal(U.bits(got), U.bits(control.get_levelset()))
        assert np.array_equal(U.bits(got), U.bits(U.prolong(uc, 32, 160).astype(np.float32).astype(np.float64)))
        same_run(fine, control)
    # coarse 32 at (32, 160), its float state ahead of the double mirror -> fine 64 at (64, 320): the exact doubles of the floats
    with capi.Context(32, 160, 1, p) as coarse, capi.Context(64, 320, 1, p) as fine:
        alone(coarse, state=32)
        coarse.set_image(U.planes_of("random", 32, 160, 1))
        coarse.set_levelset(U.smooth_levelset(32, 160))
        coarse.run(3)
        coarse.prolong_levelset_to(fine)
        uc = coarse.get_levelset()
        assert np.array_equal(uc, uc.astype(np.float32).astype(np.float64))
        assert np.array_equal(U.bits(fine.get_levelset()), U.bits(U.prolong(uc, 64, 320)))


def test_prolong_settles_the_coarse_iterations_in_flight(capi):
    p = capi.make_params(tol=0.0)
    with capi.Context(32, 72, 1, p) as coarse, capi.Context(32, 72, 1, p) as twin, capi.Context(64, 144, 1, p) as fine:
        planes = U.planes_of("random", 32, 72, 1)
        for c in (coarse, twin):
            alone(c)
            c.set_image(planes)
            c.set_levelset(U.smooth_levelset(32, 72))
            c.enqueue_steps(4)
        coarse.prolong_levelset_to(fine)               # no sync in between
        assert twin.sync()[0] == 4
        assert np.array_equal(U.bits(fine.get_levelset()), U.bits(U.prolong(twin.get_levelset(), 64, 144)))
        assert coarse.sync()[0] == 4                    # a later sync still reports them
        assert np.array_equal(U.bits(coarse.get_levelset()), U.bits(twin.get_levelset()))


def test_batches_equal_the_single_calls(capi):
    p = capi.make_params(tol=1.0)
    chans = [1, 3, 1, 3, 1]
    make = lambda coarse: [capi.Context(*(U.coarse_shape(*s) if coarse else s), c, p) for s, c in zip(U.SHAPES, chans)]
    fines, coarse_b, coarse_s, fine_b, fine_s = make(False), make(True), make(True), make(False), make(False)
    try:
        imgs = [U.planes_of("random", *s, c, seed=5) for s, c in zip(U.SHAPES, chans)]
        ucs = [U.special_levelset(*U.coarse_shape(*s), seed=9) for s in U.SHAPES]
        for f, img in zip(fines, imgs):
            f.set_image(img)
        for group in (coarse_b, coarse_s):
            for c, u in zip(group, ucs):
                c.set_levelset(u)
        n0 = launches()
        capi.restrict_image_batch(fines, coarse_b)
        assert launches() == n0 + 1                     # five pairs, ONE launch
        for f, c in zip(fines, coarse_s):
            f.restrict_image_to(c)
        for b, s, img in zip(coarse_b, coarse_s, imgs):
            assert all(np.array_equal(x, y) and np.array_equal(x, U.restrict(q)) for x, y, q in zip(b.get_image(), s.get_image(), img))
            assert b.get_stop_condition() == s.get_stop_condition()
        n0 = launches()
        capi.prolong_levelset_batch(coarse_b, fine_b)
        assert launches() == n0 + 1
        for c, f in zip(coarse_s, fine_s):
            c.prolong_levelset_to(f)
        for b, s, u, shape in zip(fine_b, fine_s, ucs, U.SHAPES):
            assert np.array_equal(U.bits(b.get_levelset()), U.bits(s.get_levelset()))
            assert np.array_equal(U.bits(b.get_levelset()), U.bits(U.prolong(u, *shape)))
    finally:
        for c in fines + coarse_b + coarse_s + fine_b + fine_s:
            c.close()


def test_errors(capi):
    L = capi.lib()
    arr = lambda *cs: (ctypes.c_void_p * len(cs))(*[c._h.value if c is not None else None for c in cs])
    text = lambda: L.cvh_last_error(None).decode()
    p = capi.make_params()
    with capi.Context(17, 33, 1, p) as f0, capi.Context(9, 17, 1, p) as c0, capi.Context(31, 50, 1, p) as f1, capi.Context(16, 25, 1, p) as c1, \
            capi.Context(16, 25, 3, p) as c1x3, capi.Context(15, 25, 1, p) as c1bad:
        img0, img1 = U.planes_of("random", 17, 33, 1), U.planes_of("random", 31, 50, 1)
        keep = U.planes_of("random", 9, 17, 1, seed=3)
        c0.set_image(keep)
        u0 = U.special_levelset(17, 33)
        f0.set_levelset(u0)
        # CVH_ERR_STATE: nothing to restrict / to prolong; pair 1 is the culprit, pair 0 is not touched
        f0.set_image(img0)
        assert L.cvh_restrict_image_batch(arr(f0, f1), arr(c0, c1), 2) == ERR_STATE and "pair 1" in text()
        c0.set_levelset(U.smooth_levelset(9, 17))
        assert L.cvh_prolong_levelset_batch(arr(c0, c1), arr(f0, f1), 2) == ERR_STATE and "pair 1" in text()
        f1.set_image(img1)
        c1.set_levelset(U.smooth_levelset(16, 25))
        for call, first, second in ((L.cvh_restrict_image_batch, (f0, f1), (c0, c1)), (L.cvh_prolong_levelset_batch, (c0, c1), (f0, f1))):
            down = call is L.cvh_restrict_image_batch
            assert call(None, arr(*second), 2) == ERR_ARG
            assert call(arr(*first), None, 2) == ERR_ARG
            assert call(arr(*first), arr(*second), 0) == ERR_ARG
            assert call(arr(first[0], None), arr(*second), 2) == ERR_ARG and "pair 1" in text()
            assert call(arr(*first), arr(second[0], None), 2) == ERR_ARG and "pair 1" in text()
            assert call(arr(first[0], first[0]), arr(*second), 2) == ERR_ARG and "pair 1" in text()       # listed twice in one list
            assert call(arr(*first), arr(second[0], first[0]), 2) == ERR_ARG and "pair 1" in text()      # across the lists
            assert call(arr(first[0]), arr(first[0]), 1) == ERR_ARG and "pair 0" in text()               # fine == coarse
            if down:
                assert call(arr(f0, f1), arr(c0, c1x3), 2) == ERR_ARG and "pair 1" in text() and "channel" in text()
                assert call(arr(f0, f1), arr(c0, c1bad), 2) == ERR_ARG and "pair 1" in text() and "16 x 25" in text()
            else:
                assert call(arr(c0, c1x3), arr(f0, f1), 2) == ERR_ARG and "pair 1" in text() and "channel" in text()
                assert call(arr(c0, c1bad), arr(f0, f1), 2) == ERR_ARG and "pair 1" in text() and "16 x 25" in text()
        if capi.device_count() > 1:
            with capi.Context(9, 17, 1, p, device=1) as far:
                assert L.cvh_restrict_image(f0._h, far._h) == ERR_ARG and "device" in text()
        # nothing was modified ...
        assert np.array_equal(c0.get_image()[0], keep[0])
        assert np.array_equal(U.bits(f0.get_levelset()), U.bits(u0))
        # ... and the contexts stay usable
        capi.restrict_image_batch([f0, f1], [c0, c1])
        assert np.array_equal(c0.get_image()[0], U.restrict(img0[0])) and np.array_equal(c1.get_image()[0], U.restrict(img1[0]))
        capi.prolong_levelset_batch([c0, c1], [f0, f1])
        assert np.array_equal(U.bits(f1.get_levelset()), U.bits(U.prolong(c1.get_levelset(), 31, 50)))


def test_driver_equals_hand_driving(capi):
    from chan_vese_amd import synth
    shapes = capi.pyramid_shapes(64, 144, 3)
    assert shapes == U.shapes(64, 144, 3) == [(64, 144), (32, 72), (16, 36)]
    img = synth.disk(64, noise=24, seed=5, h=64, w=144)
    steps = 60
    make = lambda: [alone(capi.Context(h, w, 1), resident=0, wave_pol=0) for h, w in shapes]
    dev, hand = make(), make()
    try:
        dev[0].set_option("co_resident", 1)
        dev[0].set_image([img])
        dev[-1].init_checkerboard()
        got = capi.run_coarse_to_fine(dev, steps)
        assert [c.co_resident for c in dev] == [1, 0, 0]
        hand[0].set_image([img])
        for k in range(2):
            hand[k + 1].set_image([U.restrict(q) for q in hand[k].get_image()])
        hand[-1].init_checkerboard()
        for k in (2, 1, 0):
            if k < 2:
                hand[k].set_levelset(U.prolong(hand[k + 1].get_levelset(), *shapes[k]))
            done, norm = hand[k].run(steps)
            assert (done, U.bits(np.float64(norm))) == (got[k][0], U.bits(np.float64(got[k][1]))), k
            assert np.array_equal(U.bits(hand[k].get_levelset()), U.bits(dev[k].get_levelset())), k
            assert np.array_equal(hand[k].get_image()[0], dev[k].get_image()[0]), k
        # the batch twin over two pyramids of the same image: level by level the two agree in bits, and with the single run in the mask
        single = dev[0].get_mask()
        dev[-1].init_checkerboard()
        hand[-1].init_checkerboard()
        both = capi.run_coarse_to_fine_batch([dev, hand], steps)
        assert len(both) == 2 and all(len(r) == 3 for r in both)
        assert [r[0] for r in both[0]] == [r[0] for r in both[1]]
        for a, b in zip(dev, hand):
            assert np.array_equal(U.bits(a.get_levelset()), U.bits(b.get_levelset()))
        assert U.iou(dev[0].get_mask(), single) >= 0.999     # the project's mask bar between two data flows
    finally:
        for c in dev + hand:
            c.close()


def test_finest_level_chooses_as_a_lone_context(capi):
    from chan_vese_amd import synth
    img = synth.disk(256, noise=32, seed=3)
    keys = ("kernel", "grid", "data_flow", "wave_pol")
    with capi.Context(256, 256, 1) as lone:
        lone.set_image([img])
        lone.init_checkerboard()
        want = lone.launch_info()
    levels = [capi.Context(h, w, 1) for h, w in capi.pyramid_shapes(256, 256, 3)]
    try:
        fin = levels[0]
        fin.set_image([img])
        levels[-1].init_checkerboard()
        seen = {}
        run = fin.run

        def spy(k):
            seen.update(fin.launch_info(), others=[c.co_resident for c in levels[1:]])
            return run(k)

        fin.run = spy
        capi.run_coarse_to_fine(levels, 20)
        assert {k: seen.get(k) for k in keys} == {k: want.get(k) for k in keys}
        assert seen["others"] == [0, 0]
        assert [c.co_resident for c in levels] == [1, 0, 0]
    finally:
        for c in levels:
            c.close()


def test_against_the_oracle_pyramid(capi):
    from oracle import cv_oracle as O
    img, _, want = U.oracle_proposition()
    levels = [capi.Context(h, w, 1) for h, w in capi.pyramid_shapes(256, 256, 3)]
    try:
        levels[0].set_image([img])
        levels[-1].init_checkerboard()
        got = capi.run_coarse_to_fine(levels)
        print("steps per level, finest first: device", [g[0] for g in got], "oracle", [s for _, s in want])
        for (done, _), (_, steps) in zip(got, want):
            assert abs(done - steps) <= 2
        score = U.iou(levels[0].get_mask(), O.mask(want[0][0]))
        print("finest mask IoU against the oracle pyramid:", score)
        assert score >= 0.999
    finally:
        for c in levels:
            c.close()


def test_cli_levels(capi, tmp_path):
    """bin/chan_vese --levels 3 on the oracle case's image meets the oracle pyramid's mask bar; --levels 1 and no --levels write the same
    bytes, those of a plain context's run"""
    import os
    import subprocess
    from oracle import cv_oracle as O
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "chan_vese")
    img, _, want = U.oracle_proposition()
    path = tmp_path / "disk.pgm"
    with open(path, "wb") as f:
        f.write(b"P5\n256 256\n255\n" + img.tobytes())

    def run(*args):
        r = subprocess.run([cli, "-i", str(path), "-g", *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r

    r = run("--levels", "3", "--dump-mask", str(tmp_path / "m3.pgm"), "--verbose")
    counts = [int(v) for v in r.stderr.strip().splitlines()[-1].split(":")[-1].split()]
    print("chan_vese --levels 3, steps per level finest first:", counts, "oracle", [s for _, s in want])
    assert all(abs(a - s) <= 2 for a, (_, s) in zip(counts, want))
    m3 = np.frombuffer(open(tmp_path / "m3.pgm", "rb").read()[-256 * 256:], dtype=np.uint8).reshape(256, 256) // 255
    assert U.iou(m3, O.mask(want[0][0])) >= 0.999
    run("-N", "30", "--dump-u", str(tmp_path / "u.bin"))
    run("-N", "30", "--levels", "1", "--dump-u", str(tmp_path / "u1.bin"))
    plain = open(tmp_path / "u.bin", "rb").read()
    assert plain == open(tmp_path / "u1.bin", "rb").read()
    with capi.Context(256, 256, 1) as ctx:
        ctx.set_option("math_mode", capi.MATH_FAST)
        ctx.set_image([img])
        ctx.init_checkerboard()
        ctx.run(30)
        assert plain == ctx.get_levelset().tobytes()
