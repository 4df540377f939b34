"""Level-set reinitialisation on the GPU (cvh_reinit, cvh_reinit_batch, the segmented-run helpers, Segmenter and the CLI) against the
numpy restatement of the header's definition (reinit_util.signed_edt).  The result is defined in integers and one correctly rounded
sqrt, so EVERY comparison is == on bit patterns; nothing here has a tolerance.  Run with -m gpu on an MI355X."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from chan_vese_amd import synth

import png_util
import reinit_util as R
from test_gpu_device_io import Hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 144), (144, 1), (2, 2), (3, 700), (100, 517), (64, 2016), (512, 512), (1080, 1920)]
KINDS = ["checkerboard", "after10", "rectangle", "special", "one_inside", "one_outside_corner"]


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


@pytest.fixture()
def hip(capi):
    h = Hip()
    yield h
    h.free_all()


def noisy(h, w, channels=1, seed=5):
    return [synth.disk(max(h, w), 200 - 30 * k, 50 + 20 * k, noise=32, seed=seed + k, h=h, w=w) for k in range(channels)]


def alone(ctx, **opts):
    """contexts compared in bits must not see each other in their automatic choices (tests/test_gpu_device_io.py, same_choices)"""
    ctx.set_option("co_resident", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)


def give_levelset(ctx, kind, h, w):
    if kind == "checkerboard":
        ctx.init_checkerboard()
    elif kind == "after10":
        ctx.init_checkerboard()
        ctx.run(10)
    elif kind == "rectangle":                       # the CLI's --rect: ones on exact zeros
        u = np.zeros((h, w))
        u[h // 4:max(h // 4 + 1, 3 * h // 4), w // 4:max(w // 4 + 1, 3 * w // 4)] = 1.0
        ctx.set_levelset(u)
    elif kind == "special":
        rng = np.random.default_rng(h * 10007 + w)
        u = rng.standard_normal((h, w)) * 3
        flat = u.reshape(-1)
        for k, v in enumerate([np.nan, -0.0, 1e-60, -1e-60, 0.0, 1e-45, -np.nan, np.inf, -np.inf]):
            flat[(k * 7919 + 1) % flat.size::max(flat.size // 13, 1) + k] = v
        flat[0] = 2.0                                   # both classes exist whatever the sprinkling hit
        flat[-1] = -2.0
        ctx.set_levelset(u)
    elif kind == "one_inside":
        u = np.full((h, w), -1.0)
        u[h // 2, w // 3] = 2.0
        ctx.set_levelset(u)
    elif kind == "one_outside_corner":
        u = np.full((h, w), 1.0)
        u[h - 1, w - 1] = -3.0
        ctx.set_levelset(u)
    else:
        raise ValueError(kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_definition_and_mask(capi, hip, shape, kind):
    """1 + 2: reinit() then get_levelset() is signed_edt(get_levelset() before), bit for bit; the mask is preserved and the device
    getter agrees."""
    h, w = shape
    with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image(noisy(h, w))
        give_levelset(ctx, kind, h, w)
        before, mask0 = ctx.get_levelset(), ctx.get_mask()
        assert np.array_equal(mask0.astype(bool), R.mask_of(before))
        d2, want, want_changed = R.signed_edt(before)
        changed = ctx.reinit()
        after = ctx.get_levelset()
        print(f"{h}x{w} {kind}: changed={changed} max d2={int(d2.max())} differing={int((R.bits(after) != R.bits(want)).sum())}")
        assert changed == want_changed
        assert np.array_equal(R.bits(after), R.bits(want))
        if changed:
            assert np.abs(after).min() >= 0.5
        assert np.array_equal(ctx.get_mask(), mask0)
        d_mask = hip.malloc(h * w)
        ctx.get_mask_device(d_mask)
        hip.ok(hip.L.hipDeviceSynchronize())
        assert np.array_equal(hip.get(d_mask, (h, w), np.uint8), mask0)
        # idempotent: the distance field of a distance field's mask is itself
        assert ctx.reinit() == want_changed
        assert np.array_equal(R.bits(ctx.get_levelset()), R.bits(want))
        if changed:                                                    # a new run began with the reinitialisation
            ctx.enqueue_steps(2)
            assert ctx.sync()[0] == 2


@pytest.mark.parametrize("value", [1.5, -0.25])
def test_uniform_mask_changes_nothing(capi, value):
    """3: no pixel of the other class: changed is False, the level set is untouched in bits, and the run state stays -- sync() still
    reports the iterations that had been reached."""
    h, w = 96, 160
    rng = np.random.default_rng(2)
    u = (rng.random((h, w)) + 0.5) * value
    with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image(noisy(h, w))
        ctx.set_levelset(u)
        assert ctx.reinit() is False
        assert np.array_equal(R.bits(ctx.get_levelset()), R.bits(u))
        ctx.set_params(capi.make_params(tol=0.0, dt=1e-9))            # seven tiny steps: the mask stays uniform
        ctx.enqueue_steps(7)
        assert ctx.sync()[0] == 7
        moved = ctx.get_levelset()
        assert R.mask_of(moved).all() or not R.mask_of(moved).any()
        ctx.enqueue_steps(3)                                           # in flight: reinit settles them
        assert ctx.reinit() is False
        done, _, _ = ctx.sync()
        assert done == 10
        after = ctx.get_levelset()
        assert R.mask_of(after).all() or not R.mask_of(after).any()
        ctx.enqueue_steps(2)                                           # and the run goes on where it was
        assert ctx.sync()[0] == 12


def route(capi, shape, channels, opts, via_reinit, steps=12, k=9, in_flight=False):
    """checkerboard -> `steps` iterations -> re-distance (on the device, or through the host with signed_edt) -> k iterations"""
    h, w = shape
    with capi.Context(h, w, channels, capi.make_params(tol=0.0)) as ctx:
        alone(ctx, **opts)
        ctx.set_option("trace", 64)
        ctx.set_image(noisy(h, w, channels))
        ctx.init_checkerboard()
        if in_flight and via_reinit:
            ctx.enqueue_steps(steps)                                   # NOT synced: reinit has to settle them
        else:
            ctx.enqueue_steps(steps)
            ctx.sync()
        if via_reinit:
            assert ctx.reinit() is True
        else:
            ctx.set_levelset(R.signed_edt(ctx.get_levelset())[1])
        start = ctx.get_levelset()
        ctx.enqueue_steps(k)
        done, nrm, _ = ctx.sync()
        return start, ctx.get_levelset(), ctx.get_trace(64), done, nrm


EQUIV = {
    "per-launch": ((256, 256), 1, {"resident": 0}),
    "resident": ((256, 256), 1, {"resident": 1}),
    "three channels": ((192, 320), 3, {"resident": 0}),
    "three channels resident": ((192, 320), 3, {"resident": 1}),
    "state 32": ((256, 288), 1, {"state": 32}),
}


@pytest.mark.parametrize("name", sorted(EQUIV))
@pytest.mark.parametrize("in_flight", [False, True], ids=["synced", "in flight"])
def test_equals_the_host_route(capi, name, in_flight):
    """4: context A reinit(), context B set_levelset(signed_edt(get_levelset())): the same k iterations follow, level sets and full
    traces bit for bit.  With "state" = 32 the getter's doubles are float32(signed_edt) widened."""
    shape, channels, opts = EQUIV[name]
    a = route(capi, shape, channels, opts, True, in_flight=in_flight)
    b = route(capi, shape, channels, opts, False)
    assert np.array_equal(R.bits(a[0]), R.bits(b[0]))
    if opts.get("state") == 32:
        assert np.array_equal(R.bits(a[0]), R.bits(a[0].astype(np.float32).astype(np.float64)))
    assert a[3] == b[3] == 9 and a[4] == b[4]
    assert np.array_equal(R.bits(a[1]), R.bits(b[1]))
    assert a[2].shape == b[2].shape and a[2].shape[0] == 9 and np.array_equal(R.bits(a[2]), R.bits(b[2]))


@pytest.mark.parametrize("kind", ["rectangle", "special", "one_inside"])
@pytest.mark.parametrize("shape", [(1, 9000), (3, 8200)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_wider_than_the_lds_window(capi, shape, kind):
    """Rows of more than 8192 columns are not staged in LDS: the row pass reads the distance fields from global memory.  Alone, and in
    one batch with narrow members, which then share the launch and its (full) LDS window."""
    h, w = shape
    with capi.Context(h, w, 1) as wide, capi.Context(40, 300, 1) as a, capi.Context(70, 8192, 1) as b:
        for ctx in (wide, a, b):
            give_levelset(ctx, kind, ctx.h, ctx.w)
        before = [c.get_levelset() for c in (wide, a, b)]
        want = R.signed_edt(before[0])[1]
        assert wide.reinit() is True
        got = wide.get_levelset()
        print(f"{h}x{w} {kind}: differing={int((R.bits(got) != R.bits(want)).sum())}")
        assert np.array_equal(R.bits(got), R.bits(want))
        wide.set_levelset(before[0])
        assert capi.reinit_batch([a, wide, b]) == [True, True, True]
        for c, u in zip((wide, a, b), before):
            assert np.array_equal(R.bits(c.get_levelset()), R.bits(R.signed_edt(u)[1]))


def test_planes_too_large_for_32_bit_distances_are_refused(capi):
    """h^2 + w^2 >= 2^32: CVH_ERR_ARG with a message that names the member, nothing launched, the level set untouched."""
    h, w = 65536, 1
    u = np.where(np.arange(h)[:, None] % 7 < 3, 1.0, -1.0)
    with capi.Context(h, w, 1) as big, capi.Context(16, 16, 1) as small:
        big.set_levelset(u)
        small.init_checkerboard()
        n0 = launch_sets(capi)
        with pytest.raises(capi.CvhError) as e:
            big.reinit()
        assert e.value.code == 1 and "member 0: 65536 x 1 is too large" in str(e.value)
        with pytest.raises(capi.CvhError) as e:
            capi.reinit_batch([small, big])
        assert e.value.code == 1 and "member 1: 65536 x 1 is too large" in str(e.value)
        assert launch_sets(capi) == n0
        assert np.array_equal(R.bits(big.get_levelset()), R.bits(u))
    with capi.Context(65535, 1, 1) as ok:                                      # the largest height: 65535^2 + 1 < 2^32
        v = np.full((65535, 1), -1.0)
        v[0, 0] = 1.0
        ok.set_levelset(v)
        assert ok.reinit() is True
        assert np.array_equal(R.bits(ok.get_levelset()), R.bits(R.signed_edt(v)[1]))


def launch_sets(capi):
    fn = ctypes.CDLL(capi.LIB_PATH).cvh_debug_reinit_launch_sets
    fn.restype = ctypes.c_ulong
    return fn()


def test_batch_of_mixed_members(capi):
    """5: one set of launches serves members of mixed shapes and channel counts, one of them uniform: each is bitwise its own reinit(),
    changed comes back per member."""
    specs = [((100, 517), 1, "after10"), ((64, 64), 3, "after10"), ((3, 700), 1, "rectangle"), ((96, 160), 1, "uniform"),
             ((144, 1), 1, "special"), ((256, 256), 3, "one_inside"), ((1, 144), 1, "one_outside_corner")]

    def make():
        out = []
        for (h, w), ch, kind in specs:
            ctx = capi.Context(h, w, ch, capi.make_params(tol=0.0))
            alone(ctx, resident=0)
            ctx.set_image(noisy(h, w, ch))
            if kind == "uniform":
                ctx.set_levelset(np.full((h, w), 4.0))
            else:
                give_levelset(ctx, kind, h, w)
            out.append(ctx)
        return out

    singles = make()
    before = [c.get_levelset() for c in singles]
    n0 = launch_sets(capi)
    own_changed = [c.reinit() for c in singles]
    assert launch_sets(capi) == n0 + len(specs)
    own = [c.get_levelset() for c in singles]
    for c in singles:
        c.close()
    batch = make()
    try:
        assert all(np.array_equal(R.bits(c.get_levelset()), R.bits(u)) for c, u in zip(batch, before))
        n0 = launch_sets(capi)
        changed = capi.reinit_batch(batch)
        assert launch_sets(capi) == n0 + 1                                 # ONE set of launches, not one per member
        assert changed == own_changed == [k != "uniform" for _, _, k in specs]
        for c, u, u0 in zip(batch, own, before):
            got = c.get_levelset()
            assert np.array_equal(R.bits(got), R.bits(u))
            assert np.array_equal(R.bits(got), R.bits(R.signed_edt(u0)[1]))
        done = capi.run_batch(batch[:2], 5)                                 # the members go on iterating, together or alone
        assert [d for d, _ in done] == [5, 5]
        with pytest.raises(capi.CvhError) as e:
            capi.reinit_batch([batch[0], batch[1], batch[0]])
        assert e.value.code == 1 and "member 2 duplicates member 0" in str(e.value)
    finally:
        for c in batch:
            c.close()
    with capi.Context(32, 32, 1) as fresh, capi.Context(32, 32, 1) as other:
        other.init_checkerboard()
        with pytest.raises(capi.CvhError) as e:
            fresh.reinit()
        assert e.value.code == 3
        with pytest.raises(capi.CvhError) as e:
            capi.reinit_batch([other, fresh])
        assert e.value.code == 3 and "member 1 has no level set" in str(e.value)


def hand_loop(ctx, total, every):
    steps, nrm, reinits = 0, 0.0, 0
    while steps < total:
        done, nrm = ctx.run(min(every, total - steps))
        steps += done
        if ctx.sync()[2] or steps >= total:
            break
        ctx.reinit()
        reinits += 1
    return steps, nrm, reinits


def segment_case(capi, tol, slow=False):
    """slow: eps = 0.1, dt = 1e-7, from a level set of magnitude 0.1 (a centred rectangle).  Every pixel then sits in the peak of the
    regularised delta (delta_eps(0.1) = 1.6) for the whole first segment, while after a reinitialisation |u| >= 0.5 everywhere
    (delta_eps <= 0.12, and falling with the squared distance): the norms of segment two lie far below every norm of segment one, which is
    what a stop INSIDE segment two needs.  From the checkerboard with the default parameters it is the other way round (measured norms:
    30 - 33 in segment one, 230 - 760 in segment two), and with |u| = 1e-3 too (the two region means coincide: 6e-4 against 0.15)."""
    h, w = 192, 256
    ctx = capi.Context(h, w, 1, capi.make_params(tol=tol, dt=1e-7, eps=0.1) if slow else capi.make_params(tol=tol))
    alone(ctx, resident=0)
    ctx.set_image(noisy(h, w, seed=9))
    if slow:
        u = np.full((h, w), -0.1)
        u[h // 4:3 * h // 4, w // 4:3 * w // 4] = 0.1
        ctx.set_levelset(u)
    else:
        ctx.init_checkerboard()
    return ctx


def test_run_with_reinit_is_the_hand_written_loop(capi):
    """6: run_with_reinit(ctx, 60, 20) is run(20) / reinit() / run(20) / reinit() / run(20)."""
    with segment_case(capi, 0.0) as a, segment_case(capi, 0.0) as b:
        got = capi.run_with_reinit(a, 60, 20)
        steps, nrm, reinits = hand_loop(b, 60, 20)
        assert got == (steps, nrm) and steps == 60 and reinits == 2
        assert np.array_equal(R.bits(a.get_levelset()), R.bits(b.get_levelset()))
        # every = 0 is run()
        a.init_checkerboard(); b.init_checkerboard()
        assert capi.run_with_reinit(a, 25, 0) == b.run(25)
        assert np.array_equal(R.bits(a.get_levelset()), R.bits(b.get_levelset()))


def stopping_tol(capi):
    """(tol, k): a tolerance with which the stop rule fires at iteration k of the SECOND segment of 20 and not before.  The norms of
    the tol = 0 run are read from a sibling context's trace; k is the first iteration of segment two (not its last) whose
    norm is below every earlier norm of the run by more than 2e-6 relative.  The gap makes the choice hold for a fused batch too, whose
    members agree with their own runs to 1e-9, not in bits."""
    with segment_case(capi, 0.0, True) as probe:
        probe.set_option("trace", 32)
        probe.run(20)
        first = probe.get_trace(32)[:, -1].copy()
        probe.reinit()
        probe.run(19)
        second = probe.get_trace(32)[:, -1].copy()
    with segment_case(capi, 1.0, True) as one:
        image_norm = one.get_stop_condition()                               # tol * || image ||, tol = 1
    assert len(first) == 20 and len(second) == 19
    print("norms of segment one:", first.tolist(), "segment two:", second.tolist())
    floor = first.min()
    for k in range(0, 19):
        floor = min(floor, second[k - 1]) if k else floor
        if second[k] * (1 + 2e-6) < floor:
            return float(second[k] * (1 + 1e-6) / image_norm), k + 1
    raise AssertionError("no iteration of segment two undercuts every earlier norm: pick another synthetic case")


def test_stop_inside_the_second_segment(capi):
    tol, at = stopping_tol(capi)
    with segment_case(capi, tol, True) as a, segment_case(capi, tol, True) as b:
        n0 = launch_sets(capi)
        steps, nrm = capi.run_with_reinit(a, 60, 20)
        assert steps == 20 + at and launch_sets(capi) == n0 + 1             # one reinit, none after the stop
        assert (steps, nrm) == hand_loop(b, 60, 20)[:2]
        assert np.array_equal(R.bits(a.get_levelset()), R.bits(b.get_levelset()))
    # the batch form drops the stopped member: member 0 stops in segment two, member 1 (tol 0) runs all 60
    with segment_case(capi, tol, True) as a, segment_case(capi, 0.0, True) as b:
        n0 = launch_sets(capi)
        res = capi.run_batch_with_reinit([a, b], 60, 20)
        assert [r[0] for r in res] == [20 + at, 60]
        assert launch_sets(capi) == n0 + 2                                  # both members, then member 1 alone
        assert a.sync()[0] == at and a.sync()[2]                            # member 0 still holds the run it stopped in
        assert b.sync()[0] == 20


def test_segmenter_reinit_every(capi):
    """Segmenter.segment(reinit_every=20): the masks of the batch helper's loop (one fresh child process: torch first)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reinit_child.py"), "torch"], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "reinit child ok: torch" in out.stdout


def test_cli_reinit_equals_the_python_loop(capi, tmp_path):
    """bin/chan_vese -g -s --reinit 20 -N 60 writes the selection image of the Python loop on the same PNG."""
    h, w = 120, 176
    img = synth.disk(h, 190, 60, noise=24, seed=4, h=h, w=w)
    path = tmp_path / "in.png"
    path.write_bytes(png_util.encode(png_util.pack_samples(img, 8), w, h, 8, 0, [0, 1, 2]))
    cli = os.path.join(ROOT, "bin", "chan_vese")
    r = subprocess.run([cli, "-i", str(path), "-g", "-s", "-N", "60", "-t", "0", "--reinit", "20", "--dump-u", str(tmp_path / "u.bin"),
                        "--verbose"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "chan_vese: 60 iterations" in r.stderr
    with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([img])
        ctx.init_checkerboard()
        assert capi.run_with_reinit(ctx, 60, 20)[0] == 60
        u = ctx.get_levelset()
        want = ctx.separate(np.repeat(img[:, :, None], 3, axis=2))
    assert np.array_equal(R.bits(np.fromfile(tmp_path / "u.bin", dtype=np.float64).reshape(h, w)), R.bits(u))
    got = png_util.decode8((tmp_path / "in_selection.png").read_bytes())
    assert np.array_equal(got.reshape(h, w, 3), want[:, :, ::-1])           # the file is RGB, cvh_separate's buffers BGR (gray: equal)
    # without --reinit the CLI is what it was: a different level set after the same 60 iterations
    r0 = subprocess.run([cli, "-i", str(path), "-g", "-N", "60", "-t", "0", "--dump-u", str(tmp_path / "u0.bin")], capture_output=True,
                        text=True, timeout=600)
    assert r0.returncode == 0, r0.stderr
    assert not np.array_equal(np.fromfile(tmp_path / "u0.bin", dtype=np.float64), u.reshape(-1))


@pytest.mark.parametrize("case", ["disk", "noisy"])
def test_full_size_worst_case(capi, case):
    """7: 4096 x 4096 -- the BASELINE disk's level set after 50 iterations (distances reach four digits: the row pass's worst case)
    and a noisy image's after 20.  16 whole rows (first, last, 14 seeded-random) against signed_edt's row pass behind its full column
    pass, and the packed mask of the whole plane.  The GPU work runs in a child process under its own time limit."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reinit_child.py"), "fullsize", case], capture_output=True, text=True,
                         timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert f"reinit child ok: fullsize {case}" in out.stdout
