"""Option "wave_seam" of the 2-pixel wave kernel (csv_wave2_body.inc): 1 (default) lets the final group of every strip run without the
prefetch and the park of a group that does not exist; 0 is the kernel as it was.  Which wave computes which pixel, every pixel's
arithmetic and the order of every sum are the same, so the two settings must agree BIT FOR BIT: level set, mask, every trace row
(c1, c2, norm), steps done and the stop iteration.  Anything less is a bug.

Every case forces "kernel" = 3 and "resident" = 0 and runs 6 iterations (both ping-pong parities, all four chain phases) from the same
image and level set with both settings.  Shapes are the smallest at which a path can go wrong: width 144 (a full wave-column and a
narrow one) and 272 (an odd third wave-column: its workgroup has an idle wave); equal strips of 1, 2, 3, 4, 5, 7, 8, 9 rows (shorter
than the prologue's rows, exactly one group, one group and a ragged one) in an ODD count with a ragged last strip that ends at the
image's bottom edge, the first starting at row 0; strips dealt by weight whose two strips of a workgroup differ in length."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 6
STRIP_ROWS = (1, 2, 3, 4, 5, 7, 8, 9)


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def strip_table(capi, h, tiles_x, S, strip_rows, nblocks, cls, cskew):
    fn = capi.lib().cvh_debug_strip_bounds
    fn.restype, fn.argtypes = C.c_int, [C.c_int] * 9 + [C.POINTER(C.c_int)]
    out = (C.c_int * (S + 1))()
    assert fn(3, h, tiles_x, S, strip_rows, nblocks, cls, cskew, 0, out) == 0
    return np.array(out[:], dtype=np.int64)


def planes_for(h, w, channels, seed):
    """A disk on a gradient plus noise: two regions with different means, so that c1 != c2 and the norm falls from iteration to iteration."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for k in range(channels):
        disk = ((yy - h / 2.0) ** 2 * 4 + (xx - w / 2.0) ** 2 < (w / 3.0) ** 2) * (120.0 - 30 * k)
        out.append(np.clip(40 + 20 * k + disk + xx * (30.0 / w) + rng.integers(0, 24, size=(h, w)), 0, 255).astype(np.uint8))
    return out


def run_once(capi, planes, u0, seam, opts, steps=STEPS, expect=None, **pk):
    h, w = planes[0].shape
    with capi.Context(h, w, len(planes), capi.make_params(**pk)) as ctx:
        for k, v in dict(math_mode=2, kernel=3, resident=0, trace=steps, **opts, wave_seam=seam).items():
            ctx.set_option(k, v)
        ctx.set_image(planes)
        ctx.set_levelset(u0)
        info = ctx.launch_info()
        assert info["kernel"].startswith("csv_wave2_kernel<%d, true, 3, " % len(planes)), info
        assert info["wave_seam"] == str(seam), info
        if expect is not None:
            expect(info)
        done, nrm = ctx.run(steps)
        return dict(u=ctx.get_levelset(), mask=ctx.get_mask(), trace=ctx.get_trace(steps), done=done, norm=nrm, stopped=done < steps)


def assert_same_bits(a, b, what):
    assert a["done"] == b["done"] and a["stopped"] == b["stopped"], (what, a["done"], b["done"])
    assert a["u"].dtype == np.float64 and np.array_equal(a["u"], b["u"]), (what, int((a["u"] != b["u"]).sum()))
    assert np.array_equal(a["mask"], b["mask"]), what
    assert a["trace"].shape == b["trace"].shape and np.array_equal(a["trace"], b["trace"]), (what, a["trace"], b["trace"])
    assert a["norm"] == b["norm"], what
    assert np.isfinite(a["u"]).all() and np.isfinite(a["trace"]).all(), what


def both(capi, planes, u0, opts, what, **kw):
    on = run_once(capi, planes, u0, 1, opts, **kw)
    off = run_once(capi, planes, u0, 0, opts, **kw)
    assert_same_bits(on, off, what)
    return on


def equal_strip_case(capi, sr, w):
    """(h, check of launch_info): five strips (odd: the last upper strip has no partner) of sr rows, the last one ragged."""
    h = 4 * sr + max(1, sr // 2)
    tiles_x = (w + 125) // 126

    def expect(info):
        assert int(info["strips"]) == 5 and int(info["strip_rows"]) == sr and int(info["wave_columns"]) == tiles_x, info
        b = strip_table(capi, h, tiles_x, 5, sr, int(info["grid"]), 0, 0)
        assert list(np.diff(b)) == [sr] * 4 + [max(1, sr // 2)] and b[0] == 0 and b[-1] == h, b
    return h, expect


@pytest.mark.parametrize("regime", ["far", "near"])
@pytest.mark.parametrize("sync", [0, 1])
@pytest.mark.parametrize("state", [64, 32])
@pytest.mark.parametrize("channels", [1, 3])
def test_short_strips_same_bits(capi, channels, state, sync, regime):
    """Strips of 1 .. 9 rows, both widths, one and three channels, FP64 and FP32 state, with and without the workgroup barrier per group, the
    far regime (dt = 1: the checkerboard's |u| leaves the near field at once) and the all-near regime (dt = 0.001: near-form groups)."""
    pk = dict(tol=0.0, dt=0.001 if regime == "near" else 1.0)
    if channels == 3:
        pk.update(lambda1=[1, 0.8, 0.5], lambda2=[0.7, 0.5, 1], nu=0.01)
    for i, sr in enumerate(STRIP_ROWS):
        w = (144, 272)[(i + channels + sync) & 1]
        h, expect = equal_strip_case(capi, sr, w)
        planes = planes_for(h, w, channels, 1000 * sr + w)
        u0 = capi.checkerboard_host(h, w)
        opts = dict(wave_cls=0, strip_rows=sr, wave_sync=sync, state=state)
        r = both(capi, planes, u0, opts, (sr, w, channels, state, sync, regime), expect=expect, **pk)
        assert r["done"] == STEPS and not r["stopped"]


@pytest.mark.parametrize("channels,h,strips", [(1, 1000, 90), (3, 1000, 90), (1, 4900, 600)])
def test_unequal_pairs_same_bits(capi, channels, h, strips):
    """Strips dealt by cumulative weight ("strips" = an exact count with the class-major numbering): 144 x 1000 in 90 strips of 11 or 12 rows, and
    144 x 4900 in 600 strips = 300 workgroups, more than one dispatch round, so that the class skew gives the rounds different strip lengths.  In
    both the two strips of some workgroups differ in length (the shorter one's wave waits at the remaining barriers)."""
    w = 144
    seen = {}

    def expect(info):
        assert int(info["strips"]) == strips, info
        for cskew in (500, 425, 0):   # whichever skew the host applied: the pairs differ under each
            ln = np.diff(strip_table(capi, h, 2, strips, int(info["strip_rows"]), (strips + 1) // 2, 32, cskew))
            assert ln.min() >= 1 and any(ln[k] != ln[k + 1] for k in range(0, len(ln) - 1, 2)), (cskew, ln)
        seen["ok"] = True
    planes = planes_for(h, w, channels, 77)
    u0 = capi.checkerboard_host(h, w)
    pk = dict(tol=0.0) if channels == 1 else dict(tol=0.0, lambda1=[1, 0.8, 0.5], lambda2=[0.7, 0.5, 1])
    both(capi, planes, u0, dict(strips=strips, wave_sync=1), ("unequal", channels, h), expect=expect, **pk)
    assert seen["ok"]


def test_stop_inside_the_run_same_iteration(capi):
    """tol > 0, placed from the norms of a tol = 0 run so that the stop rule (norm <= tol x ||I||) fires inside the run: same stop iteration."""
    sr, w = 5, 272
    h, expect = equal_strip_case(capi, sr, w)
    planes = planes_for(h, w, 1, 5)
    u0 = capi.checkerboard_host(h, w)
    opts = dict(wave_cls=0, strip_rows=sr)
    free = run_once(capi, planes, u0, 0, opts, steps=12, expect=expect, tol=0.0)
    norms = free["trace"][:, -1]
    assert len(norms) == 12
    k = next((i for i in range(2, 11) if norms[i] < norms[:i].min()), None)
    assert k is not None, norms
    threshold = np.sqrt(norms[k] * norms[:k].min())          # between the smallest norm before iteration k and iteration k's
    tol = threshold / np.sqrt((planes[0].astype(np.float64) ** 2).sum())
    r = both(capi, planes, u0, opts, "stop", steps=12, tol=float(tol))
    assert r["stopped"] and 2 < r["done"] < 12, (r["done"], k, norms)


def test_fused_batch_members_same_bits(capi):
    """Two contexts through cvh_enqueue_steps_batch (csv_wave2_batch_kernel), each against its own "wave_seam" = 0 run."""
    shapes = [(4 * 7 + 3, 272), (4 * 7 + 3, 272)]
    res = {}
    for seam in (1, 0):
        ctxs = []
        try:
            for m, (h, w) in enumerate(shapes):
                ctx = capi.Context(h, w, 1, capi.make_params(tol=0.0))
                ctxs.append(ctx)
                for k, v in dict(math_mode=2, kernel=3, resident=0, trace=STEPS, wave_cls=0, strip_rows=7, wave_seam=seam).items():
                    ctx.set_option(k, v)
                ctx.set_image(planes_for(h, w, 1, 300 + m))
                ctx.set_levelset(capi.checkerboard_host(h, w) * (1.0 + 0.25 * m))
            capi.enqueue_steps_batch(ctxs, STEPS)
            out = []
            for ctx in ctxs:
                total, nrm, stopped = ctx.sync()
                out.append(dict(u=ctx.get_levelset(), mask=ctx.get_mask(), trace=ctx.get_trace(STEPS), done=total, norm=nrm, stopped=stopped))
            res[seam] = out
        finally:
            for ctx in ctxs:
                ctx.close()
    for m in range(len(shapes)):
        assert res[1][m]["done"] == STEPS
        assert_same_bits(res[1][m], res[0][m], ("batch member", m))
    assert not np.array_equal(res[1][0]["u"], res[1][1]["u"])


def test_beyond_the_wide_store_hazard_size_same_bits(capi):
    """1024 x 1008: beyond the size at which the wide-store hazard of DESIGN.md 4.1 showed; default geometry, every row compared."""
    h, w = 1024, 1008
    planes = planes_for(h, w, 1, 9)
    u0 = capi.checkerboard_host(h, w)
    r = both(capi, planes, u0, {}, "1024x1008", tol=0.0)
    assert r["done"] == STEPS
