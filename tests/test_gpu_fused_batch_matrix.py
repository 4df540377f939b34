"""Fused batch, member by member: every member of a batch is checked against one of two bars.

- Bits (own run): with pinned strips ("strip_rows"), level set bytes, every trace row, steps_done and stopped equal the same
  context's own per-launch run (resident = 0).
- Oracle: with the automatic (share) geometry, oracle.csv_run with the member's OWN parameters and image -- level set <= 1e-9 max|u|,
  every trace row rtol 1e-9, mask exact, steps_done and the stop iteration equal (fused_batch_util.assert_oracle).

The members differ where a mix-up between them would show: parameters (every CvhStepArgs coefficient, eps and the far-field series, the
stop condition, sum_img, lambdas), geometry (the batch-only share geometry and its edges), flavour (chain / no chain, STRICT, FP32 state,
near regime, channels) and schedule (table rotation, member order and leader, flushes at a grid change)."""
import numpy as np
import pytest

from fused_batch_util import (KBATCH_OWN_ROWS, STRICT, assert_oracle, assert_same, cone, data_flow, first_stop_at_or_after, last_grid,
                              member, num_cus, planes, result, share)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def f32(a):
    return a.astype(np.float32).astype(np.float64)


def close_all(ctxs):
    for c in ctxs:
        c.close()


@pytest.fixture
def pool():
    """The contexts a test creates, closed at teardown even after a failed assertion: a context left open would make every later test's
    context part of a batch (the automatic flow steps aside for one)."""
    ctxs = []
    yield ctxs
    close_all(ctxs)


def stop_tol(capi, ctx, want, steps, pk, u0):
    """(tol, k): tol at which the member's own stop rule fires at k, the first clean stop iteration >= want of its tol = 0 run."""
    ctx.set_params(capi.make_params(**dict(pk, tol=1.0)))
    ctx.set_levelset(u0)
    scale = ctx.get_stop_condition()          # ||mean_k I_k||_2 (tol = 1)
    ctx.set_params(capi.make_params(**dict(pk, tol=0.0)))
    ctx.set_levelset(u0)
    assert ctx.run(steps)[0] == steps
    norms = ctx.get_trace(steps)[:, -1]
    k = first_stop_at_or_after(norms, want)
    return norms[k - 1] / scale * (1 + 1e-6), k


# ---- 1. different parameters per member ----

# every coefficient distinct; members 0 and 1 share shape and image (one group, one representative: bg.rep is member 0's arguments)
PARAMS = [dict(mu=0.5, nu=0.0, dt=0.5, eps=1.0), dict(mu=0.3, nu=0.01, dt=0.8, eps=1.5),
          dict(mu=0.7, nu=-0.02, dt=0.3, eps=0.7, lambda1=[1.0, 0.8, 0.5], lambda2=[0.7, 0.5, 1.0]),
          dict(mu=0.2, nu=0.03, dt=1.0, eps=2.0, lambda1=[0.6, 1.0, 0.9], lambda2=[1.0, 0.4, 0.8]),
          dict(mu=0.45, nu=0.005, dt=0.6, eps=1.2), dict(mu=0.6, nu=-0.01, dt=0.4, eps=0.8), dict(mu=0.35, nu=0.02, dt=0.7, eps=1.1)]
SPECS = [(256, 256, 1, {}, 60), (256, 256, 1, {}, 60), (200, 384, 3, {}, 62), (160, 272, 3, {}, 63), (144, 528, 1, {"kernel": 3}, 64),
         (97, 300, 1, {}, 65), (512, 512, 1, {}, 66)]
WANT_STOP = [8, 13, None, 11, None, 16, None]     # None: a tol that never fires (still distinct: stop_cond differs per member)


def test_members_with_different_parameters(capi, oracle, pool):
    """Seven members, every one with its own mu / nu / dt / eps / tol (3-channel members: own lambda1 / lambda2 per channel); members 0 and 1
    are the same shape and image, so they are one group launched with member 0's arguments as the representative and differ ONLY in
    CvhStepArgs (alpha, beta, gamma, eps, inv_eps, dk1 / dk2, far_k / far_thr, stop_cond).  Both bars, then the reverse order (another
    leader, other table offsets): the same bits per member."""
    steps = 20
    ctxs = [member(capi, h, w, ch, dict(opts, resident=0), seed=seed, **PARAMS[i]) for i, (h, w, ch, opts, seed) in enumerate(SPECS)]
    pool.extend(ctxs)
    imgs = [planes(h, w, ch, seed) for h, w, ch, _, seed in SPECS]
    u0 = [cone(h, w) for h, w, *_ in SPECS]
    assert ctxs[0].launch_info()["kernel"] == ctxs[1].launch_info()["kernel"]
    assert ctxs[4].launch_info()["kernel"].startswith("csv_wave2_kernel<1") and ctxs[5].launch_info()["kernel"].startswith("csv_wave_kernel<1")
    pks, ks = [], []
    for i, c in enumerate(ctxs):
        if WANT_STOP[i]:
            tol, k = stop_tol(capi, c, WANT_STOP[i], steps, PARAMS[i], u0[i])
        else:
            tol, k = 1e-12 * (i + 1), None
        pks.append(dict(PARAMS[i], tol=tol))
        ks.append(k)
        c.set_params(capi.make_params(**pks[-1]))
    # automatic geometry: the oracle with each member's own parameters
    for c, u in zip(ctxs, u0):
        c.set_levelset(u)
    out = capi.run_batch(ctxs, steps)
    first = []
    for i, c in enumerate(ctxs):
        done = assert_oracle(oracle, c, imgs[i], u0[i], pks[i], steps, ("member", i), done=out[i][0])
        assert done == (ks[i] or steps), (i, done, ks[i])
        first.append(result(c, steps))
    # reverse order: member 6 leads, member 0 is the last of its group
    order = list(range(len(ctxs)))[::-1]
    for c, u in zip(ctxs, u0):
        c.set_levelset(u)
    capi.run_batch([ctxs[i] for i in order], steps)
    for i, c in enumerate(ctxs):
        assert_same(result(c, steps), first[i], ("reverse order", i))
    # pinned strips: the bits of each member's own run
    for c in ctxs:
        c.set_option("strip_rows", 16)
        c.set_levelset(cone(c.h, c.w))
    capi.run_batch(ctxs, steps)
    fused = [result(c, steps) for c in ctxs]
    for i, c in enumerate(ctxs):
        c.set_levelset(u0[i])
        c.run(steps)
        assert_same(fused[i], result(c, steps), ("own run, strip_rows 16", i))
    close_all(ctxs)


# ---- 2. batch-only geometries ----

# (name, h, w, channels, options); the big members make the small ones' shares tiny
GEOM = [("big0", 1024, 1024, 1, {}), ("big1", 1024, 1024, 1, {}), ("wide", 150, 1008, 1, {"kernel": 3}), ("clamp", 13, 1008, 1, {"kernel": 3}),
        ("row", 1, 144, 1, {}), ("col", 144, 1, 1, {}), ("tiny", 2, 2, 1, {"chain": 0}), ("thin", 3, 700, 1, {}), ("odd", 37, 53, 1, {}),
        ("c3", 100, 517, 3, {})]


def test_batch_only_geometries(capi, oracle, pool):
    """The share geometry of csv_batch.hip (batch_share, then resolve_geometry with the share as the CU count), with num_cus from the device.
    On the MI355X (256 CUs) and sum n = 2 x 1024^2 + 150 x 1008 + 13 x 1008 + 144 + 144 + 4 + 2100 + 1961 + 51700 = 2,317,509 pixels:
      clamp 13 x 1008 (2-pixel): share = round(256 x 13104 / 2317509) = round(1.45) = 1 CU; wave-columns 8, nbc = 4,
            nstrips = 2 x ((1 x 3) / 4) = 0 -> clamped to 1: ONE strip of 13 rows holds the whole plane (tiles_y = 1, odd);
      wide  150 x 1008 (2-pixel): share = round(16.7) = 17; nstrips = 2 x (51 / 4) = 24, 150 / 24 -> 7 rows -> 8: tiles_y = 19 (odd),
            10 strip pairs, the last with one strip;
      tiny  2 x 2, chain = 0: 1 workgroup, no bookkeeper: a section of exactly 1 workgroup (7 of padding);
      row   1 x 144: share 1, 1 strip of 3 wave-columns: 1 workgroup + the bookkeeper (6 of padding);
      col   144 x 1: share 1, nstrips = 5 (1 CU x 5 waves per SIMD): 29-row strips, 5 workgroups + bookkeeper;
      thin  3 x 700: 12 wave-columns, 3 workgroups; odd 37 x 53: 5 strips of 8 rows; c3 100 x 517 x 3: share 6, 6 strips of 17 rows;
      wave_imgv is off for every width that is not a multiple of 16 (53, 517, 700, 1) and w < 144 takes the 1-pixel kernel.
    Every member: the oracle bar, and the grid it ran on is the predicted one.  clamp and wide: the same strip_rows on an own run gives the
    same geometry, and the same bits."""
    steps = 12
    ctxs = [member(capi, h, w, ch, dict(opts, resident=0), seed=70 + i, trace=steps, nu=0.01, dt=0.5) for i, (_, h, w, ch, opts) in enumerate(GEOM)]
    pool.extend(ctxs)
    cus = num_cus(capi, ctxs[0])
    tot = sum(h * w for _, h, w, _, _ in GEOM)
    pred = {}
    for name, h, w, ch, opts in GEOM:
        own = data_flow(capi, h, w, ch, kernel=opts.get("kernel", -1), cus=cus)
        s = share(cus, h * w, tot) if own[3] < KBATCH_OWN_ROWS else 0
        pred[name] = (s,) + (data_flow(capi, h, w, ch, kernel=opts.get("kernel", -1), cus=s) if s else own)
    if cus == 256:   # the arithmetic of the docstring (another CU count still runs every bar below with its own shares)
        assert pred["clamp"][0] == 1 and pred["clamp"][3:5] == (1, 13) and 2 * ((1 * 3) // ((pred["clamp"][2] + 1) // 2)) == 0, pred["clamp"]
        assert pred["wide"][0] == 17 and pred["wide"][1] == 3 and pred["wide"][3] == 19, pred["wide"]
        assert pred["tiny"][5] == 1 and pred["row"][5] == 1 and pred["col"][3:5] == (5, 29), (pred["tiny"], pred["row"], pred["col"])
        assert pred["c3"][0] == 6 and pred["c3"][3] == 6, pred["c3"]
    assert pred["clamp"][1] == 3 and pred["clamp"][3] % 2 == 1 and pred["wide"][3] % 2 == 1      # odd tiles_y in the 2-pixel kernel
    # (row 0 and column 0 of the checkerboard are zeros: planes of 1 or 2 rows / columns start from a seeded random level set instead)
    rng = np.random.default_rng(7)
    u0 = [np.ascontiguousarray(oracle.checkerboard(h, w)) if min(h, w) > 2 else rng.normal(size=(h, w)) for _, h, w, _, _ in GEOM]
    for c, u in zip(ctxs, u0):
        c.set_levelset(u)
    out = capi.run_batch(ctxs, steps)
    fused = {}
    for i, (name, h, w, ch, opts) in enumerate(GEOM):
        assert last_grid(capi, ctxs[i]) == pred[name][5], (name, last_grid(capi, ctxs[i]), pred[name])
        assert_oracle(oracle, ctxs[i], planes(h, w, ch, 70 + i), u0[i], dict(tol=0, nu=0.01, dt=0.5), steps, name, done=out[i][0])
        fused[name] = result(ctxs[i], steps)
    for name in ("clamp", "wide"):
        i = [g[0] for g in GEOM].index(name)
        c = ctxs[i]
        c.set_option("strip_rows", pred[name][4])
        info = c.launch_info()
        assert int(info["strips"]) == pred[name][3] and int(info["strip_rows"]) == pred[name][4], (name, info, pred[name])
        c.set_levelset(u0[i])
        c.run(steps)
        assert_same(result(c, steps), fused[name], (name, "own run on the share geometry's strips"))
    close_all(ctxs)


# ---- 3. member flavours mixed in one batch ----

NEAR = dict(tol=0, dt=0.001, nu=-3.0)
FLAV = [("fast_chain", 256, 256, 1, {}, {}), ("fast_nochain", 256, 256, 1, {"chain": 0}, {}),
        ("strict_k2", 200, 300, 1, {"math_mode": STRICT}, {}), ("strict_2px", 144, 528, 1, {"math_mode": STRICT, "kernel": 3}, {}),
        ("st32", 64, 528, 1, {"state": 32}, {}), ("st32_twin", 64, 528, 1, {"kernel": 3}, {}),
        ("near_on", 150, 528, 1, {"kernel": 3}, NEAR), ("near_off", 150, 528, 1, {"kernel": 3, "near_switch": 0}, NEAR),
        ("c3_1px", 100, 517, 3, {}, dict(lambda1=[1, 0.8, 0.5], lambda2=[0.7, 0.5, 1])), ("c3_2px", 150, 528, 3, {"kernel": 3}, {})]


def test_member_flavours_in_one_batch(capi, oracle, pool):
    """One batch: a FAST chain member and a chain = 0 member of the same instantiation (one group; chain / chain_phase / partials are per member),
    STRICT on kernel 2 and on the 2-pixel kernel, an FP32-state member (state32, the float buffers) and its FP64 twin (same image, same u0), the
    near regime (dt = 0.001: |u| < 32 eps all run) with near_switch 1 and 0, one and three channels.  Bars: the oracle; the FP32-state member
    the float-rounded oracle of test_gpu_state32.py.  Six iterations: from this checkerboard the FP64 flows' own runs drift from the oracle by
    1.3e-10 after 4 iterations and 1.5e-9 after 8 (every kernel alike, batch or not), past the 1e-9 bar."""
    steps = 6
    base = dict(tol=0, nu=0.01, dt=0.5)
    ctxs, pks = [], []
    for i, (name, h, w, ch, opts, pk) in enumerate(FLAV):
        pks.append(dict(base, **pk))
        seed = 80 + i if name != "st32_twin" else 80 + i - 1
        ctxs.append(member(capi, h, w, ch, dict(opts, resident=0), seed=seed, trace=steps, **pks[-1]))
        pool.append(ctxs[-1])
    names = [f[0] for f in FLAV]
    k = {n: ctxs[names.index(n)].launch_info()["kernel"] for n in names}
    assert k["fast_chain"] == k["fast_nochain"] and ctxs[1].launch_info()["chain"] == "0" and ctxs[0].launch_info()["chain"] == "1"
    assert k["strict_k2"].startswith("csv_wave_kernel<1, false") and k["strict_2px"].startswith("csv_wave2_kernel<1, false")
    assert k["st32"].startswith("csv_wave2_kernel<1, true") and k["st32"].endswith("true>") and k["st32_twin"].endswith("false>")
    assert k["c3_1px"].startswith("csv_wave_kernel<3") and k["c3_2px"].startswith("csv_wave2_kernel<3")
    u0 = []
    rng = np.random.default_rng(8)
    u32 = f32(rng.normal(scale=3.0, size=(64, 528)))       # float-representable: the FP32 state starts from u0 itself
    for name, h, w, *_ in FLAV:
        u0.append(u32 if name.startswith("st32") else np.ascontiguousarray(oracle.checkerboard(h, w)))
    for c, u in zip(ctxs, u0):
        c.set_levelset(u)
    out = capi.run_batch(ctxs, steps)
    assert [d for d, _ in out] == [steps] * len(ctxs)
    for i, (name, h, w, ch, opts, pk) in enumerate(FLAV):
        imgs = planes(h, w, ch, 80 + i if name != "st32_twin" else 80 + i - 1)
        if name == "st32":
            u_f = u0[i].copy()
            p = oracle.make_params(**pks[i])
            for _ in range(steps):
                oracle.csv_step(imgs, u_f, p)
                u_f = f32(u_f)
            u_g = ctxs[i].get_levelset()
            assert np.array_equal(u_g, f32(u_g))
            scale = np.abs(u_f).max()
            assert np.abs(u_g - u_f).max() <= 2e-5 * scale, np.abs(u_g - u_f).max() / scale
            assert (ctxs[i].get_mask() != oracle.mask(u_f)).mean() <= 1e-4
            continue
        assert_oracle(oracle, ctxs[i], imgs, u0[i], pks[i], steps, name)
        if name.startswith("near"):
            assert np.abs(ctxs[i].get_levelset()).max() < 32.0          # the regime this member is about
    close_all(ctxs)


# ---- 4. schedules ----

SCHED_MEMBERS = [(256, 256, 1, {}, dict(mu=0.5, nu=0.01, dt=0.5)), (200, 384, 3, {}, dict(mu=0.3, nu=0.0, dt=0.8, eps=1.3)),
                 (144, 528, 1, {"kernel": 3}, dict(mu=0.6, nu=-0.01, dt=0.4)), (128, 200, 1, {"chain": 0}, dict(mu=0.4, nu=0.02, dt=0.6, eps=0.9))]
# (kind, members, iterations): "b" a fused enqueue, "o" an own enqueue; lengths 1, 3, 5, 2 (table rotation), subsets and orders (leaders c, b, d, a)
SCHEDULE = [("b", "abcd", 1), ("b", "cad", 3), ("o", "b", 2), ("b", "bdac", 5), ("b", "db", 0), ("b", "a", 2), ("b", "dcba", 2)]


def run_schedule(capi, ctxs, syncs):
    by = dict(zip("abcd", ctxs))
    for c in ctxs:
        c.init_checkerboard()
        c.reset_run()
    for kind, who, n in SCHEDULE:
        group = [by[x] for x in who]
        if kind == "b":
            capi.enqueue_steps_batch(group, n)
        else:
            group[0].enqueue_steps(n)
        if syncs:
            for c in group:
                c.sync()
    return [result(c, 16) for c in ctxs]


def test_schedules_rotation_subsets_and_leaders(capi, oracle, pool):
    """Batch enqueues of 1, 3, 5 and 2 iterations (the cached tables rotate by bc->rot; a non-multiple of 4 leaves them mid-period), subsets and
    orders that change the leader and the tables, an own enqueue of one member in between (its grid differs: flush_for_grid), an enqueue of 0
    and a batch of one.  No sync: each member equals the oracle for its total count; with pinned strips, the bits of the same sequence with
    a sync after every step (automatic geometry too)."""
    totals = {x: sum(n for _, who, n in SCHEDULE if x in who) for x in "abcd"}
    assert totals == {"a": 13, "b": 10, "c": 11, "d": 11}
    ctxs = [member(capi, h, w, ch, dict(opts, resident=0), seed=90 + i, trace=16, tol=0, **pk) for i, (h, w, ch, opts, pk) in enumerate(SCHED_MEMBERS)]
    pool.extend(ctxs)
    free = run_schedule(capi, ctxs, False)
    for i, (x, c) in enumerate(zip("abcd", ctxs)):
        h, w, ch, opts, pk = SCHED_MEMBERS[i]
        assert free[i][2] == totals[x] and not free[i][3], (x, free[i][2:])
        assert_oracle(oracle, c, planes(h, w, ch, 90 + i), oracle.checkerboard(h, w), dict(pk, tol=0), totals[x], x)
    synced = run_schedule(capi, ctxs, True)
    for i, x in enumerate("abcd"):
        assert_same(free[i], synced[i], (x, "automatic geometry"))
    for c in ctxs:
        c.set_option("strip_rows", 16)
    free = run_schedule(capi, ctxs, False)
    synced = run_schedule(capi, ctxs, True)
    for i, x in enumerate("abcd"):
        assert free[i][2] == totals[x]
        assert_same(free[i], synced[i], (x, "strip_rows 16"))
    close_all(ctxs)


# ---- 5. stops on every boundary ----

def boundary_sequence(capi, main, others, syncs, n=(8, 12, 8)):
    main.set_levelset(cone(main.h, main.w))
    main.reset_run()
    for o in others:
        o.init_checkerboard()
        o.reset_run()

    def settle(ctxs):
        if syncs:
            for c in ctxs:
                c.sync()

    main.enqueue_steps(n[0])                                   # own, per launch: the own grid
    settle([main])
    capi.enqueue_steps_batch([others[0], main] + others[1:], n[1])   # the share grid; main is not the leader
    settle([main] + others)
    main.enqueue_steps(n[2])                                   # own again: the own grid
    settle([main])
    for o in others:
        o.sync()
    return result(main, sum(n))


def test_stops_on_every_flow_boundary(capi, oracle, pool):
    """main (512^2, per-launch own flow) runs 8 own iterations, 12 fused beside two 1024^2 members (its share grid differs from its own:
    both transitions go through flush_for_grid), 8 own.  The stop is placed on iteration 8 (last own before the batch), 9 (first fused),
    20 (last fused) and 21 (first own after): with and without syncs the same bits, steps_done = the oracle's stop iteration.  Then
    run_batch(ctxs, -1) with every member at tol > 0, each stopping at its own iteration."""
    pk = dict(nu=0.01, dt=0.5)
    main = member(capi, 512, 512, seed=100, opts={"resident": 0}, **pk)
    others = [member(capi, 1024, 1024, seed=101 + i, **pk) for i in range(2)]
    pool.extend([main] + others)
    cus = num_cus(capi, main)
    own = data_flow(capi, 512, 512, cus=cus)
    s = share(cus, 512 * 512, 512 * 512 + 2 * 1024 * 1024)
    fused_grid = data_flow(capi, 512, 512, cus=s)[4]
    assert own[3] < KBATCH_OWN_ROWS and fused_grid != own[4], (own, s, fused_grid)   # the batch runs main on another grid
    main.set_params(capi.make_params(tol=0.0, **pk))
    ref = boundary_sequence(capi, main, others, True)
    assert ref[2] == 28 and not ref[3]
    norms = ref[1][:, -1]
    main.set_params(capi.make_params(tol=1.0, **pk))
    scale = main.get_stop_condition()
    img = planes(512, 512, 1, 100)
    for k in (8, 9, 20, 21):
        assert norms[:k - 1].min() > norms[k - 1] * (1 + 1e-5), (k, norms[:k])
        tol = norms[k - 1] / scale * (1 + 1e-6)
        main.set_params(capi.make_params(tol=tol, **pk))
        synced = boundary_sequence(capi, main, others, True)
        free = boundary_sequence(capi, main, others, False)
        assert synced[2] == k and synced[3], (k, synced[2:])
        assert_same(free, synced, ("stop at", k))
        assert_oracle(oracle, main, img, cone(512, 512), dict(pk, tol=tol), 28, ("stop at", k), done=free[2])
    close_all([main] + others)
    # run_batch(-1): every member stops, each at its own iteration
    specs = [(256, 256, 1, {}, 7, dict(nu=0.01, dt=0.5)), (200, 384, 3, {}, 12, dict(nu=0.0, dt=0.7)), (144, 528, 1, {"kernel": 3}, 17, dict(nu=0.01, dt=0.4))]
    ctxs = [member(capi, h, w, ch, dict(opts, resident=0), seed=110 + i, **pk) for i, (h, w, ch, opts, _, pk) in enumerate(specs)]
    pool.extend(ctxs)
    pks, ks = [], []
    for c, (h, w, ch, opts, want, pk) in zip(ctxs, specs):
        tol, k = stop_tol(capi, c, want, 30, pk, cone(h, w))
        pks.append(dict(pk, tol=tol))
        ks.append(k)
        c.set_params(capi.make_params(**pks[-1]))
        c.set_levelset(cone(h, w))
    assert len(set(ks)) == len(ks)
    out = capi.run_batch(ctxs, -1)
    assert [d for d, _ in out] == ks, (out, ks)
    for i, (c, (h, w, ch, *_)) in enumerate(zip(ctxs, specs)):
        assert_oracle(oracle, c, planes(h, w, ch, 110 + i), cone(h, w), pks[i], 40, ("run_batch -1", i), done=out[i][0])
    close_all(ctxs)
