"""Component measures on the GPU (cvh_measure*) against the numpy restatement of the header's definition (measure_util).  Every field of a
row is an integer, so EVERY comparison is ==.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import components_util as cu
import measure_util as mu
from test_gpu_components import levelset, make

pytestmark = pytest.mark.gpu
SHAPES = [(1, 144), (144, 1), (2, 2), (33, 257), (100, 517), (64, 2016)]
KINDS = ["rand50", "spiral", "comb", "isolated", "inside", "outside", "special"]
CLEAN_SETS = [(5, 0, 0), (0, -1, 0), (4, -1, 1)]
ERR_ARG, ERR_STATE = 1, 3   # cvh_status


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def want_table(ctx, conn, invert, clean=(0, 0, 0)):
    f = cu.foreground(ctx.get_levelset(), invert)
    return mu.measure_clean(f, ctx.get_image(), conn, clean[0], clean[1], bool(clean[2]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_table_is_the_restatement(capi, shape, kind):
    """both connectivities, both classes, one and three channels with distinct noisy planes: K and every integer field; with (0, 0, 0) the
    first six fields are cvh_components' table; cap < K, cap = 0 and the count alone"""
    h, w = shape
    for channels in (1, 3):
        with make(capi, h, w, kind, channels) as ctx:
            for conn in (4, 8):
                for invert in (False, True):
                    want = want_table(ctx, conn, invert)
                    k, got = ctx.measure(conn, invert)
                    print(f"{h}x{w} {kind} C={channels} conn {conn} invert {invert}: K = {k} (restatement {want.size})")
                    assert k == want.size
                    mu.assert_tables_equal(got, want, (conn, invert))
            kc, comp = ctx.components(8, True)   # conn 8, inverted: the last table above
            assert kc == k
            six = np.zeros(got.size, comp.dtype)
            for f in comp.dtype.names:
                six[f] = got[f]
            assert six.tobytes() == comp.tobytes()   # byte for byte
            for cap in (k // 2, 0, k + 3):
                k2, part = ctx.measure(8, True, cap=cap)
                assert k2 == k
                mu.assert_tables_equal(part, want[:min(cap, k)], cap)
            count = capi.C.c_int(-1)
            assert capi.lib().cvh_measure(ctx._h, 8, 1, 0, 0, 0, None, 0, capi.C.byref(count), None) == 0 and count.value == k
            assert capi.lib().cvh_measure(ctx._h, 8, 1, 0, 0, 0, None, 0, None, None) == 0


@pytest.mark.parametrize("shape,channels", [((2, 40000), 3), ((40000, 2), 1), ((1, 65535), 1)], ids=lambda v: str(v))
def test_long_planes_all_inside(capi, shape, channels):
    """c^2 fits 32 bits at these widths and the sum of two squares does not: a 32-bit partial anywhere shows here"""
    h, w = shape
    with make(capi, h, w, "inside", channels) as ctx:
        want = want_table(ctx, 4, False)
        k, got = ctx.measure(4, False)
        assert k == 1 and int(want["sxx"][0]) == h * ((w - 1) * w * (2 * w - 1) // 6) and int(want["syy"][0]) == w * ((h - 1) * h * (2 * h - 1) // 6)
        print(f"{h}x{w}: sxx {int(got['sxx'][0])} syy {int(got['syy'][0])} sxy {int(got['sxy'][0])} perimeter {int(got['perimeter'][0])}")
        mu.assert_tables_equal(got, want)
        mu.assert_shapes_match(capi.region_shapes(got, channels), got, channels)


def test_too_wide_is_refused(capi):
    with make(capi, 1, 65536, "inside") as ctx:
        with pytest.raises(capi.CvhError) as e:
            ctx.measure(cap=0)
        assert e.value.code == ERR_ARG and "member 0: 1 x 65536 is too large" in str(e.value)
        assert ctx.components(cap=0)[0] == 1   # (the context stays usable)


@pytest.mark.parametrize("kind", ["rand50", "spiral", "special"])
@pytest.mark.parametrize("shape", [(33, 257), (100, 517)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_cleaned_masks(capi, shape, kind):
    """the table of a cleaned mask is the restatement's on components_util.clean(...); the level set's own class is untouched"""
    h, w = shape
    with make(capi, h, w, kind, 3) as ctx:
        for conn, invert in ((4, False), (8, True)):
            for clean in CLEAN_SETS:
                want = want_table(ctx, conn, invert, clean)
                k, got = ctx.measure(conn, invert, *clean)
                print(f"{h}x{w} {kind} conn {conn} invert {invert} {clean}: K = {k} (restatement {want.size})")
                assert k == want.size
                mu.assert_tables_equal(got, want, (conn, invert, clean))
                if clean[2]:
                    assert k <= 1
        mu.assert_tables_equal(ctx.measure(4, False)[1], want_table(ctx, 4, False))


def test_batch_of_mixed_members(capi):
    """four members of mixed shapes and channel counts, one of them without a component: each table == the member's own call"""
    specs = [(100, 517, 1, "rand50"), (33, 257, 3, "spiral"), (64, 2016, 1, "outside"), (144, 1, 3, "special")]
    ctxs = [make(capi, h, w, kind, ch) for h, w, ch, kind in specs]
    try:
        for args in ((4, False, 0, 0, False), (8, True, 0, 0, False), (4, False, 4, -1, True)):
            own = [c.measure(*args) for c in ctxs]
            got = capi.measure_batch(ctxs, *args)
            assert [k for k, _ in got] == [k for k, _ in own]
            for (k, t), (_, t_own) in zip(got, own):
                mu.assert_tables_equal(t, t_own, args)
                assert t.tobytes() == t_own.tobytes()
            if args[0] == 4 and not args[2]:
                assert got[2][0] == 0 and got[2][1].size == 0   # the member without a component, beside the others
            caps = [3, 0, 5, 1]
            for (k, t), (k_own, t_own), cap in zip(capi.measure_batch(ctxs, *args, cap=caps), own, caps):
                assert k == k_own and t.tobytes() == t_own[:cap].tobytes()
        with pytest.raises(capi.CvhError) as e:
            capi.measure_batch(ctxs + ctxs[:1], cap=0)
        assert e.value.code == ERR_ARG and "member 4 duplicates member 0" in str(e.value)
    finally:
        for c in ctxs:
            c.close()


def test_sums_follow_the_smoothed_planes(capi):
    """after Perona-Malik s1 and s2 are those of the planes get_image returns"""
    h, w = 100, 517
    with make(capi, h, w, "rand50", 3) as ctx:
        before = ctx.measure(8, False)[1]
        raw = [p.copy() for p in ctx.get_image()]
        ctx.perona_malik(K=30, L=0.25, T=2.0)
        planes = ctx.get_image()
        assert any(not np.array_equal(a, b) for a, b in zip(raw, planes))
        want = mu.measure(cu.foreground(ctx.get_levelset()), planes, 8)
        got = ctx.measure(8, False)[1]
        mu.assert_tables_equal(got, want)
        assert not np.array_equal(got["s1"], before["s1"]) and np.array_equal(got["sxx"], before["sxx"])


def test_the_call_only_reads(capi):
    """20 iterations with a measure (raw and cleaned) in the middle end in the same level-set bytes as 20 without"""
    h, w = 128, 256
    res = []
    for interrupt in (False, True):
        with make(capi, h, w, "checkerboard") as ctx:
            ctx.run(10)
            if interrupt:
                k, t = ctx.measure(4, False)
                mu.assert_tables_equal(t, want_table(ctx, 4, False))
                ctx.measure(8, False, 4, -1, True)
            steps, _ = ctx.run(10)
            res.append((steps, ctx.get_levelset().tobytes(), tuple(p.tobytes() for p in ctx.get_image())))
    assert res[0] == res[1]


def test_iterations_in_flight_are_settled(capi):
    h, w = 100, 517
    res = []
    for sync_first in (False, True):
        with make(capi, h, w, "checkerboard") as ctx:
            ctx.enqueue_steps(6)
            if sync_first:
                ctx.sync()
            res.append(ctx.measure(8, False)[1].tobytes())
    assert res[0] == res[1]


def test_refusals(capi):
    h, w = 33, 257
    with make(capi, h, w, "rand50") as ctx:
        bad = [(lambda: ctx.measure(5), "conn must be 4 or 8"), (lambda: ctx.measure(4, False, -1), "min_area must not be negative"),
               (lambda: ctx.measure(4, False, 0, -2), "fill_holes must be -1"), (lambda: ctx.measure(4, False, 0, 0, 2), "keep_largest must be 0 or 1")]
        for call, msg in bad:
            with pytest.raises(capi.CvhError) as e:
                call()
            assert e.value.code == ERR_ARG and msg in str(e.value), (msg, str(e.value))
        row = np.zeros(1, capi.REGION_DTYPE)
        assert capi.lib().cvh_measure(ctx._h, 4, 0, 0, 0, 0, row.ctypes.data, -1, None, None) == ERR_ARG
        assert b"cap must not be negative" in capi.lib().cvh_last_error(ctx._h)
        with capi.Context(8, 8, 1, capi.make_params()) as no_image:
            no_image.set_levelset(levelset("inside", 8, 8))
            with pytest.raises(capi.CvhError) as e:
                no_image.measure()
            assert e.value.code == ERR_STATE and "member 0 has no image" in str(e.value)
            with pytest.raises(capi.CvhError) as e:
                capi.measure_batch([ctx, no_image], cap=0)
            assert e.value.code == ERR_STATE and "cvh_measure_batch: member 1 has no image" in str(e.value)
        with capi.Context(8, 8, 1, capi.make_params()) as no_levelset:
            no_levelset.set_image([np.zeros((8, 8), np.uint8)])
            with pytest.raises(capi.CvhError) as e:
                capi.measure_batch([ctx, no_levelset], cap=0)
            assert e.value.code == ERR_STATE and "member 1 has no level set" in str(e.value)
        mu.assert_tables_equal(ctx.measure()[1], want_table(ctx, 4, False))
