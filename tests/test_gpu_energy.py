"""The energy calls on the GPU (include/chanvese_hip.h, "Energy"; chan_vese_amd/csrc/energy_kernels.hip): every term against the numpy
restatement (energy_util.py, exactly rounded sums) to 1e-9 relative -- the bar c1 / c2 / norm are held to against exact sums: a term is
a sum of non-negative products of a few correctly rounded or few-ulp operations --, c1 / c2 against cvh_get_means bit for bit, the
batch against its members bit for bit, the read-only promise for every kernel flavour, "state" = 32, the descent along a run on the
card against the oracle's series (1e-6 relative: the free-run bar of DESIGN.md section 5), the plateau driver, and every refusal.

Shapes: the pyramid's (pyramid_util.SHAPES): one lane-tail (16 x 16), odd sides (17 x 33, 31 x 50), one width the 2-pixel CSV kernel
takes (64 x 144: two column pieces, two row bands), and several pieces per row with a one-column last piece (33 x 257: lane 0 alone,
its right neighbour the clamped column).  NOT covered: h * w >= 2^32 and contexts on two devices (the sibling calls' tests say why).
Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import energy_util as E

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_STATE = 0, 1, 3
CASES = [(h, w, ch) for (h, w) in E.SHAPES for ch in E.CHANNELS]


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def params_of(channels):
    """one channel: the defaults but tol; three: every parameter the total weighs moved off its default"""
    if channels == 1:
        return dict(tol=0.0)
    return dict(tol=0.0, mu=0.4, nu=0.01, eps=1.5, lambda1=[1, 0.8, 0.5], lambda2=[0.7, 0.5, 1])


def restated(ctx, planes, u, pk, e):
    """the restatement for the level set u with the means the card used"""
    kw = {k: v for k, v in pk.items() if k != "tol"}
    return E.terms(planes, u, c1=e.c1, c2=e.c2, **kw)


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """two capi.Energy, every field bit for bit (a NaN equals itself)"""
    return all(np.array_equal(bits(getattr(a, f)), bits(getattr(b, f))) for f in ("total", "length", "area", "fit_in", "fit_out", "c1", "c2"))


def check_terms(e, want, what):
    got, ref = E.flat(e), E.flat(want)
    print(what, " ".join(f"{g:.17g}/{r:.17g}" for g, r in zip(got, ref)))
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (what, got, ref)          # non-finite exactly where the restatement's are
    assert np.all(np.abs(got[fin] - ref[fin]) <= 1e-9 * np.abs(ref[fin])), (what, got, ref, np.abs(got - ref) / np.abs(ref))


def levelsets(capi, h, w):
    """name -> level set (None: the one 5 iterations of a run from the checkerboard leave)"""
    return {"smooth": E.smooth_levelset(h, w), "checkerboard": capi.checkerboard_host(h, w), "run5": None,
            "all_inside": np.full((h, w), 3.0), "all_outside": np.full((h, w), -40.0),
            "planted": E.planted_levelset(h, w), "infinities": E.inf_levelset(h, w)}


# ---- 1. terms against the restatement; c1 / c2 against cvh_get_means ----
@pytest.mark.parametrize("h,w,channels", CASES)
def test_terms_match_the_restatement(capi, h, w, channels):
    pk = params_of(channels)
    with capi.Context(h, w, channels, capi.make_params(**pk)) as ctx:
        for kind in ("random", "all0", "all255"):
            planes = E.planes_of(kind, h, w, channels)
            ctx.set_image(planes)
            for name, u in levelsets(capi, h, w).items():
                if u is None:
                    ctx.init_checkerboard()
                    assert ctx.run(5)[0] == 5
                    u = ctx.get_levelset()
                else:
                    ctx.set_levelset(u)
                e = ctx.energy()                       # (a level set just set: the means are taken inside the call; after a run: the state block's)
                c1, c2 = ctx.get_means()
                assert np.array_equal(bits(e.c1), bits(c1)) and np.array_equal(bits(e.c2), bits(c2)), (kind, name, e, c1, c2)
                assert same_bits(ctx.energy(), e), (kind, name)        # now from the state block cvh_get_means filled: the same bits
                assert np.array_equal(bits(ctx.get_levelset()), bits(u))
                check_terms(e, restated(ctx, planes, u, pk, e), f"{h}x{w}x{channels} {kind} {name}")
                if name in ("planted",):
                    assert not np.isfinite(E.flat(e)).any()


def test_constant_inputs_give_exact_terms(capi):
    """a constant u has length 0 exactly, u = 0 has area h w / 2 exactly, planes of zeros have every fit term 0 exactly"""
    h, w = 33, 257
    with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image(E.planes_of("all0", h, w, 1))
        ctx.set_levelset(np.zeros((h, w)))
        e = ctx.energy()
        assert e.length == 0.0 and e.area == h * w / 2 and e.fit_in == (0.0,) and e.fit_out == (0.0,) and e.total == 0.0
        ctx.set_levelset(np.full((h, w), -2.5))
        assert ctx.energy().length == 0.0


# ---- 2. the batch ----
def test_batch_equals_its_members_bit_for_bit(capi):
    raw = C.CDLL(capi.LIB_PATH)
    raw.cvh_debug_energy_launch_sets.restype = C.c_ulong
    ctxs = []
    try:
        for i, (h, w, ch) in enumerate(CASES):
            ctx = capi.Context(h, w, ch, capi.make_params(**params_of(ch)))
            ctxs.append(ctx)
            ctx.set_image(E.planes_of("random", h, w, ch, seed=i))
            if i % 3 == 0:
                ctx.init_checkerboard()
                ctx.run(3)                                # the means in the state block
            elif i % 3 == 1:
                ctx.set_levelset(E.smooth_levelset(h, w))  # the means taken inside the call
            else:
                ctx.set_levelset(E.planted_levelset(h, w))
        alone = [c.energy() for c in ctxs]
        before = raw.cvh_debug_energy_launch_sets()
        together = capi.energy_batch(ctxs)
        assert raw.cvh_debug_energy_launch_sets() == before + 1     # one set of launches for the ten members
        again = capi.energy_batch(ctxs)
        backwards = capi.energy_batch(ctxs[::-1])[::-1]              # another leader, other sections of the grid
        some = capi.energy_batch(ctxs[3:7])
        for i, e in enumerate(alone):
            assert same_bits(together[i], e) and same_bits(again[i], e) and same_bits(backwards[i], e), (CASES[i], together[i], e)
        assert all(same_bits(a, b) for a, b in zip(some, alone[3:7]))
    finally:
        for c in ctxs:
            c.close()


# ---- 3. read-only ----
FLAVOURS = {"tile": ({"kernel": 0, "resident": 0}, "csv_step_kernel"), "wave": ({"kernel": 2, "resident": 0}, "csv_wave_kernel"),
            "wave2": ({"kernel": 3, "resident": 0}, "csv_wave2_kernel"), "resident": ({"resident": 1}, "csv_resident_kernel")}


@pytest.mark.parametrize("in_flight", [False, True])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_energy_only_reads(capi, flavour, in_flight):
    """7 iterations, the energy, 9 more: level set, trace, means and sync() are those of a context that made the same calls but the
    energy's (two cvh_run calls are two runs of 7 and 9 iterations; two cvh_enqueue_steps calls one run of 16)"""
    h, w = 64, 144
    options, kernel = FLAVOURS[flavour]
    planes = E.planes_of("random", h, w, 1, seed=5)
    planes[0][16:48, 40:100] //= 3
    out = []
    for with_energy in (True, False):
        with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx:
            for k, v in options.items():
                ctx.set_option(k, v)
            ctx.set_option("trace", 16)
            ctx.set_image(planes)
            ctx.set_levelset(E.smooth_levelset(h, w))
            assert ctx.launch_info()["kernel"].startswith(kernel), ctx.launch_info()
            seen = []
            if with_energy:
                seen.append(ctx.energy())                 # before the run: the means are taken beside the state block
            first = None
            if in_flight:
                ctx.enqueue_steps(7)                      # left in flight: the call settles them, as the getters do
            else:
                assert ctx.run(7)[0] == 7
                first = bits(ctx.get_trace(16))           # (cvh_run begins a run of its own: the second one's rows replace these)
            if with_energy:
                seen.append(ctx.energy())
                seen.append(ctx.energy())
                assert same_bits(seen[1], seen[2])
            if in_flight:
                ctx.enqueue_steps(9)
            else:
                assert ctx.run(9)[0] == 9
            state = ctx.sync()
            out.append((bits(ctx.get_levelset()), bits(ctx.get_trace(16)), state, bits(np.concatenate(ctx.get_means())), first))
    assert out[0][2] == out[1][2] and out[0][2][0] == (16 if in_flight else 9), (out[0][2], out[1][2])
    assert len(out[0][1]) == out[0][2][0] and (in_flight or len(out[0][4]) == 7)
    for a, b in zip(out[0], out[1]):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, b), flavour
    # and of a context that ran the 16 iterations in one piece, with no energy call
    with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx:
        for k, v in options.items():
            ctx.set_option(k, v)
        ctx.set_option("trace", 16)
        ctx.set_image(planes)
        ctx.set_levelset(E.smooth_levelset(h, w))
        if in_flight:
            ctx.enqueue_steps(16)
        else:
            assert ctx.run(16)[0] == 16
        state = ctx.sync()
        straight = (bits(ctx.get_levelset()), bits(ctx.get_trace(16)), state, bits(np.concatenate(ctx.get_means())))
    assert np.array_equal(out[0][0], straight[0]) and np.array_equal(out[0][3], straight[3]) and out[0][2][1:] == state[1:], flavour
    rows = out[0][1] if in_flight else np.concatenate([out[0][4], out[0][1]])
    assert np.array_equal(rows, straight[1]), flavour


# ---- 4. "state" = 32 ----
@pytest.mark.parametrize("channels", E.CHANNELS)
def test_state32_energy_is_of_the_float_level_set(capi, channels):
    h, w = 64, 144
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    pk = params_of(channels)
    planes = E.planes_of("random", h, w, channels, seed=9)
    u0 = E.smooth_levelset(h, w) * (1 + 1e-9)             # not float-representable
    assert not np.array_equal(u0, f32(u0))
    with capi.Context(h, w, channels, capi.make_params(**pk)) as ctx:
        ctx.set_option("state", 32)
        ctx.set_image(planes)
        ctx.set_levelset(u0)
        e = ctx.energy()
        check_terms(e, restated(ctx, planes, f32(u0), pk, e), f"state32 x{channels} start")
        c1, c2 = ctx.get_means()
        assert np.array_equal(bits(e.c1), bits(c1)) and np.array_equal(bits(e.c2), bits(c2))
        assert ctx.run(3)[0] == 3
        e = ctx.energy()
        u = ctx.get_levelset()
        assert np.array_equal(u, f32(u))
        check_terms(e, restated(ctx, planes, u, pk, e), f"state32 x{channels} after 3")


# ---- 5. descent on the card ----
def test_energy_falls_along_a_run_on_the_card(capi, oracle):
    img, want = E.oracle_series(64)
    with capi.Context(64, 64, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([img])
        ctx.init_checkerboard()
        series = {0: ctx.energy()}
        steps, _, every_step = capi.run_monitored(ctx, max_steps=E.SAMPLES[-1], every=1)
        assert steps == E.SAMPLES[-1] and [s for s, _ in every_step] == list(range(1, steps + 1))
        series.update(dict(every_step))
    got = [series[s].total for s in E.SAMPLES]
    ref = [t["total"] for _, t in want]
    print(" ".join(f"{s}:{g:.9e}/{r:.9e}" for s, g, r in zip(E.SAMPLES, got, ref)))
    assert all(b < a for a, b in zip(got, got[1:])), got
    assert all(abs(g - r) <= 1e-6 * abs(r) for g, r in zip(got, ref)), [abs(g - r) / abs(r) for g, r in zip(got, ref)]


def test_rel_plateau_ends_at_the_first_segment_that_meets_it(capi):
    from chan_vese_amd import synth
    img = synth.disk(64, noise=32, seed=3)
    x = 3e-3
    with capi.Context(64, 64, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([img])
        ctx.init_checkerboard()
        steps, norm, series = capi.run_monitored(ctx, max_steps=512, every=16, rel_plateau=x)
        assert ctx.sync()[1] == norm and not ctx.sync()[2]
        assert same_bits(ctx.energy(), series[-1][1])
    tot = [e.total for _, e in series]
    print(steps, " ".join(f"{s}:{v:.6e}" for (s, _), v in zip(series, tot)))
    assert [s for s, _ in series] == list(range(16, steps + 1, 16)) and 32 <= steps < 512
    met = [abs(a - b) <= x * abs(a) for a, b in zip(tot, tot[1:])]
    assert met[-1] and not any(met[:-1]), met                     # the first segment that meets it, not a later one
    # every <= 0: exactly run(max_steps) plus one final energy
    with capi.Context(64, 64, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([img])
        ctx.init_checkerboard()
        steps0, _, series0 = capi.run_monitored(ctx, max_steps=steps, every=0)
        assert steps0 == steps and [s for s, _ in series0] == [steps]
        assert abs(series0[0][1].total - tot[-1]) <= 1e-9 * tot[-1]


def test_run_batch_monitored_members_leave(capi):
    """three members of two shapes: each member's series is its own run_monitored's, and a plateaued member leaves the batch"""
    from chan_vese_amd import synth
    imgs = [synth.disk(64, noise=32, seed=3), synth.disk(64, 200, 50, noise=8, seed=4, h=48, w=80), synth.disk(64, noise=32, seed=5)]
    kw = dict(max_steps=96, every=16, rel_plateau=1.5e-2)
    make = lambda img: capi.Context(img.shape[0], img.shape[1], 1, capi.make_params(tol=0.0))
    ctxs = [make(img) for img in imgs]
    try:
        for c, img in zip(ctxs, imgs):
            c.set_option("resident", 0)
            c.set_image([img])
            c.init_checkerboard()
        res = capi.run_batch_monitored(ctxs, **kw)
        for (steps, norm, series), c in zip(res, ctxs):
            assert steps == series[-1][0] and c.sync()[1] == norm and same_bits(c.energy(), series[-1][1])
            tot = [e.total for _, e in series]
            met = [abs(a - b) <= kw["rel_plateau"] * abs(a) for a, b in zip(tot, tot[1:])]
            assert not any(met[:-1]) and (met[-1] if steps < kw["max_steps"] else True), (steps, tot)
        print([r[0] for r in res])
        assert len({r[0] for r in res}) > 1 or res[0][0] < kw["max_steps"]      # somebody left before the budget was spent
    finally:
        for c in ctxs:
            c.close()


# ---- 6. refusals ----
def test_refusals(capi):
    L = capi.lib()
    h, w = 16, 25
    mk = lambda ch=1: capi.Context(h, w, ch, capi.make_params(tol=0.0))
    ready, ready3, no_image, no_levelset = mk(), mk(3), mk(), mk()
    try:
        for c, ch in ((ready, 1), (ready3, 3)):
            c.set_image(E.planes_of("random", h, w, ch))
            c.init_checkerboard()
        no_image.set_levelset(E.smooth_levelset(h, w))
        no_levelset.set_image(E.planes_of("random", h, w, 1))
        before = [c.energy() for c in (ready, ready3)]
        out = (capi.EnergyTerms * 4)()
        arr = lambda *cs: (C.c_void_p * max(len(cs), 1))(*[c._h.value if c is not None else None for c in cs])
        err = lambda: L.cvh_last_error(None).decode()
        cases = [
            (lambda: L.cvh_energy_batch(None, 2, out), ERR_ARG, "cvh_energy_batch: empty member list"),
            (lambda: L.cvh_energy_batch(arr(ready, ready3), 0, out), ERR_ARG, "cvh_energy_batch: empty member list"),
            (lambda: L.cvh_energy_batch(arr(ready, ready3), -1, out), ERR_ARG, "cvh_energy_batch: empty member list"),
            (lambda: L.cvh_energy_batch(arr(ready, None, ready3), 3, out), ERR_ARG, "cvh_energy_batch: member 1 is NULL"),
            (lambda: L.cvh_energy_batch(arr(ready, ready3), 2, None), ERR_ARG, "cvh_energy_batch: out is NULL"),
            (lambda: L.cvh_energy_batch(arr(ready, ready3, ready), 3, out), ERR_ARG, "cvh_energy_batch: member 2 duplicates member 0"),
            (lambda: L.cvh_energy_batch(arr(ready, ready3, no_image), 3, out), ERR_STATE, "cvh_energy_batch: member 2 has no image"),
            (lambda: L.cvh_energy_batch(arr(ready, no_levelset, ready3), 3, out), ERR_STATE, "cvh_energy_batch: member 1 has no level set"),
            (lambda: L.cvh_energy(no_image._h, out), ERR_STATE, "cvh_energy: member 0 has no image"),
            (lambda: L.cvh_energy(no_levelset._h, out), ERR_STATE, "cvh_energy: member 0 has no level set"),
            (lambda: L.cvh_energy(ready._h, None), ERR_ARG, "cvh_energy: out is NULL"),
        ]
        for call, code, text in cases:
            assert call() == code, (text, err())
            assert err().startswith(text), (text, err())
        assert L.cvh_energy(None, out) == ERR_ARG
        with pytest.raises(capi.CvhError) as ex:
            capi.energy_batch([ready, no_levelset])
        assert "member 1 has no level set" in str(ex.value)
        # everybody is as usable as before
        after = capi.energy_batch([ready, ready3])
        assert all(same_bits(a, b) for a, b in zip(before, after))
        no_image.set_image(E.planes_of("random", h, w, 1))
        no_levelset.init_checkerboard()
        assert np.isfinite(E.flat(no_image.energy())).all() and same_bits(no_levelset.energy(), ready.energy())
        assert ready.run(2)[0] == 2
    finally:
        for c in (ready, ready3, no_image, no_levelset):
            c.close()
