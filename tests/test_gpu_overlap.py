"""Component overlaps on the GPU (cvh_overlaps*) against the numpy restatement of the header's definition (overlap_util).  Every field of a
row is an integer and the order of the rows is defined, so EVERY comparison is == on P, K and the bytes.  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import components_util as cu
import overlap_util as ou
from test_gpu_components import levelset, make
from test_gpu_device_io import Hip

pytestmark = pytest.mark.gpu
# runs that cross a wave's 64 lanes and a row end; 96 x 96 is two workgroups (8192 pixels each, 32 trips of 256 lanes); 100 x 517 is
# seven, the last one partial: every lane makes second trips, and the last trip of the plane is ragged
SHAPES = [(1, 1), (1, 200), (200, 1), (7, 65), (33, 129), (96, 96), (100, 517)]
ERR_ARG, ERR_STATE = 1, 3   # cvh_status
EXTREMES = np.array([-1, -2 ** 31, 2 ** 31 - 1, 0], np.int64)


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


def other_plane(kind, h, w):
    rng = np.random.default_rng(h * 31 + w)
    if kind == "grid":
        return ou.grid_labels(h, w, 8)
    if kind == "few":      # long runs of equal keys, some across row ends
        return np.repeat(rng.integers(-3, 4, (h * w + 36) // 37), 37)[:h * w].reshape(h, w).astype(np.int32)
    if kind == "extremes":
        return EXTREMES[rng.integers(0, EXTREMES.size, (h, w))].astype(np.int32)
    if kind == "const":
        return np.full((h, w), 7, np.int32)
    if kind == "index":
        return (np.arange(h * w, dtype=np.int64) + 1).reshape(h, w).astype(np.int32)
    raise ValueError(kind)


def want_rows(ctx, other, conn=4, invert=False, clean=(0, 0, 0)):
    return ou.overlaps(cu.foreground(ctx.get_levelset(), invert), other, conn, clean[0], clean[1], bool(clean[2]))


def launches(capi):
    fn = capi.lib().cvh_debug_overlap_launch_sets
    fn.restype = capi.C.c_ulong
    return fn()


@pytest.mark.parametrize("kind", ["rand50", "spiral", "isolated"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rows_are_the_restatement(capi, hip, shape, kind):
    """conn 4 and 8, invert, four kinds of B (the signed order among them): P, K and every byte; the host form == the device form; two
    calls in a row give equal bytes; counts add up to h w"""
    h, w = shape
    with make(capi, h, w, kind) as ctx:
        for b_kind, conn, invert in (("grid", 4, False), ("few", 8, False), ("extremes", 4, True), ("grid", 8, True)):
            other = other_plane(b_kind, h, w)
            want, k_want = want_rows(ctx, other, conn, invert)
            got, k = ctx.overlaps(other, conn, invert)
            print(f"{h}x{w} {kind} B={b_kind} conn {conn} invert {invert}: P = {got.size} K = {k} (restatement {want.size}, {k_want})")
            assert k == k_want
            ou.assert_rows_equal(got, want, (b_kind, conn, invert))
            assert int(got["count"].astype(np.int64).sum()) == h * w
            d = hip.upload(other)
            dev, k_dev = ctx.overlaps(d, conn, invert)
            again, _ = ctx.overlaps(d, conn, invert)
            assert k_dev == k and dev.tobytes() == got.tobytes() == again.tobytes()


def test_areas_are_cvh_measure_s(capi):
    with make(capi, 100, 517, "rand50", 3) as ctx:
        rows, k = ctx.overlaps(other_plane("grid", 100, 517), 8)
        k2, regions = ctx.measure(8)
        assert k == k2
        areas = np.zeros(k + 1, np.int64)
        np.add.at(areas, rows["a"], rows["count"])
        assert np.array_equal(areas[1:], regions["area"].astype(np.int64))


def test_all_background_and_wholly_inside(capi):
    h, w = 96, 96
    with make(capi, h, w, "outside") as ctx:
        rows, k = ctx.overlaps(other_plane("grid", h, w))
        assert k == 0 and rows.size == 144 and not rows["a"].any()
        ou.assert_rows_equal(rows, want_rows(ctx, other_plane("grid", h, w))[0])
    for shape in ((96, 96), (100, 517)):   # the contended case: every run of the plane adds to ONE pair
        with make(capi, *shape, "inside") as ctx:
            rows, k = ctx.overlaps(other_plane("const", *shape))
            assert k == 1 and rows.size == 1 and tuple(rows[0]) == (1, 7, shape[0] * shape[1], 0)


def test_the_table_grows(capi):
    """96 x 96 with B = flat index + 1 on a checkerboard-like mask: 9216 pairs of one pixel; a fresh context's 4096 slots overflow, so the
    pair launch runs more than once -- and once only in the next call, which finds the table grown"""
    h, w = 96, 96
    with make(capi, h, w, "isolated") as ctx:
        other = other_plane("index", h, w)
        before = launches(capi)
        rows, k = ctx.overlaps(other, 4, False, cap=h * w)
        first = launches(capi) - before
        print(f"pair launches of the first call: {first}; K = {k}")
        assert first >= 2
        assert rows.size == h * w and (rows["count"] == 1).all() and k == (h // 2) * (w // 2)
        ou.assert_rows_equal(rows, want_rows(ctx, other)[0])
        before = launches(capi)
        again, _ = ctx.overlaps(other, 4, False, cap=h * w)
        assert launches(capi) - before == 1 and again.tobytes() == rows.tobytes()
        small, _ = ctx.overlaps(other_plane("const", h, w))   # a small table in the grown one
        ou.assert_rows_equal(small, want_rows(ctx, other_plane("const", h, w))[0])


def test_cap_gives_a_prefix(capi):
    h, w = 33, 129
    with make(capi, h, w, "rand50") as ctx:
        other = other_plane("grid", h, w)
        want, k_want = want_rows(ctx, other)
        P = want.size
        for cap in (0, 1, P - 1, P, P + 5):
            table = np.full(max(cap, 1), 0x55, np.uint8).repeat(16).view(capi.OVERLAP_DTYPE)[:max(cap, 1)].copy()
            pairs, count = capi.C.c_long(-1), capi.C.c_int(-1)
            rc = capi.lib().cvh_overlaps(ctx._h, 4, 0, 0, 0, 0, other.ctypes.data, table.ctypes.data, cap, capi.C.byref(pairs), capi.C.byref(count))
            assert rc == 0 and pairs.value == P and count.value == k_want
            assert table[:min(cap, P)].tobytes() == want[:cap].tobytes()
            assert (table[min(cap, P):].view(np.uint8) == 0x55).all()   # nothing behind the prefix is written
        assert capi.lib().cvh_overlaps(ctx._h, 4, 0, 0, 0, 0, other.ctypes.data, None, 0, None, None) == 0   # every output may be NULL


@pytest.mark.parametrize("clean", [(5, 0, 0), (0, -1, 0), (0, 3, 0), (4, -1, 1), (0, 0, 1)], ids=str)
def test_cleaned_masks(capi, clean):
    """a mask with speckle and holes: rows == the restatement on components_util.clean(...), areas == cvh_measure's"""
    h, w = 100, 517
    with make(capi, h, w, "rand60") as ctx:
        other = other_plane("grid", h, w)
        for conn, invert in ((4, False), (8, True)):
            want, k_want = want_rows(ctx, other, conn, invert, clean)
            got, k = ctx.overlaps(other, conn, invert, *clean)
            print(f"conn {conn} invert {invert} {clean}: P = {got.size} K = {k} (restatement {want.size}, {k_want})")
            assert k == k_want
            ou.assert_rows_equal(got, want, (conn, invert, clean))
            k2, regions = ctx.measure(conn, invert, *clean)
            areas = np.zeros(k + 1, np.int64)
            np.add.at(areas, got["a"], got["count"])
            assert k2 == k and np.array_equal(areas[1:], regions["area"].astype(np.int64))
        ou.assert_rows_equal(ctx.overlaps(other)[0], want_rows(ctx, other)[0])   # the level set's own class is untouched


def test_float_state(capi):
    """ "state" = 32 (it needs a width that is a multiple of 16 and >= 144): the class comes from the float state, ten iterations ahead
    of the double mirror when the call arrives"""
    h, w = 65, 160
    with make(capi, h, w, "after10", state=32) as ctx:
        other = other_plane("few", h, w)
        got, k = ctx.overlaps(other, 8)
        want, k_want = want_rows(ctx, other, 8)
        assert k == k_want
        ou.assert_rows_equal(got, want)
    with make(capi, h, w, "special", state=32) as ctx:
        got, k = ctx.overlaps(other, 4, True)
        want, k_want = want_rows(ctx, other, 4, True)
        assert k == k_want
        ou.assert_rows_equal(got, want)


def test_batch_of_mixed_members(capi, hip):
    """the shapes above with mixed channel counts: each member's rows == the member's own call, byte for byte, also in reversed order;
    per-member caps; a member without a table"""
    specs = [(h, w, 1 + 2 * (i % 2), ("rand50", "spiral", "outside", "inside")[i % 4]) for i, (h, w) in enumerate(SHAPES)]
    ctxs = [make(capi, h, w, kind, ch) for h, w, ch, kind in specs]
    try:
        others = [other_plane(("grid", "few", "extremes")[i % 3], c.h, c.w) for i, c in enumerate(ctxs)]
        ptrs = [hip.upload(o) for o in others]
        for args in ((4, False, 0, 0, False), (8, True, 0, 0, False), (4, False, 4, -1, True)):
            own = [c.overlaps(o, *args) for c, o in zip(ctxs, others)]
            for (rows, k), o, c in zip(own, others, ctxs):
                want, k_want = want_rows(c, o, args[0], args[1], args[2:])
                assert k == k_want
                ou.assert_rows_equal(rows, want, args)
            got = capi.overlaps_batch(ctxs, ptrs, *args)
            back = capi.overlaps_batch(ctxs[::-1], ptrs[::-1], *args)[::-1]
            for (r, k), (r2, k2), (r_own, k_own) in zip(got, back, own):
                assert k == k2 == k_own and r.tobytes() == r2.tobytes() == r_own.tobytes()
            caps = [3, 0, 5, 1, 10 ** 6, 2, 0]
            for (r, k), (r_own, k_own), cap in zip(capi.overlaps_batch(ctxs, ptrs, *args, cap=caps), own, caps):
                assert k == k_own and r.tobytes() == r_own[:cap].tobytes()
        # tables NULL, and a NULL entry beside a table
        n = len(ctxs)
        pairs, counts = (capi.C.c_long * n)(), (capi.C.c_int * n)()
        members, addr = capi._member_array(ctxs), capi._address_array(ptrs, n)
        assert capi.lib().cvh_overlaps_device_batch(members, n, 4, 0, 0, 0, 0, addr, None, None, pairs, counts, None) == 0
        own = [c.overlaps(o) for c, o in zip(ctxs, others)]
        assert [pairs[i] for i in range(n)] == [r.size for r, _ in own] and [counts[i] for i in range(n)] == [k for _, k in own]
        table = np.zeros(own[1][0].size, capi.OVERLAP_DTYPE)
        tptrs = (capi.C.c_void_p * n)(*[table.ctypes.data if i == 1 else None for i in range(n)])
        caps = (capi.C.c_long * n)(*[table.size if i == 1 else -5 for i in range(n)])   # (read only for the member with a table)
        assert capi.lib().cvh_overlaps_device_batch(members, n, 4, 0, 0, 0, 0, addr, tptrs, caps, None, None, None) == 0
        assert table.tobytes() == own[1][0].tobytes()
    finally:
        for c in ctxs:
            c.close()


def test_the_call_only_reads(capi):
    """40 iterations with the call (raw and cleaned, host and grown table) in the middle end in the same level-set bytes as 40 without"""
    h, w = 128, 256
    res = []
    for interrupt in (False, True):
        with make(capi, h, w, "checkerboard") as ctx:
            ctx.run(20)
            if interrupt:
                other = other_plane("grid", h, w)
                ou.assert_rows_equal(ctx.overlaps(other)[0], want_rows(ctx, other)[0])
                ctx.overlaps(other_plane("index", h, w), 8, False, 4, -1, True)
            steps, _ = ctx.run(20)
            res.append((steps, ctx.get_levelset().tobytes(), tuple(p.tobytes() for p in ctx.get_image())))
    assert res[0] == res[1]


def test_iterations_in_flight_are_settled_and_no_image_is_needed(capi):
    h, w = 100, 517
    other = other_plane("grid", h, w)
    res = []
    for sync_first in (False, True):
        with make(capi, h, w, "checkerboard") as ctx:
            ctx.enqueue_steps(6)
            if sync_first:
                ctx.sync()
            res.append(ctx.overlaps(other, 8)[0].tobytes())
    assert res[0] == res[1]
    with capi.Context(8, 8, 1, capi.make_params()) as no_image:
        no_image.set_levelset(levelset("inside", 8, 8))
        rows, k = no_image.overlaps(np.zeros((8, 8), np.int32))
        assert k == 1 and [tuple(r) for r in rows] == [(1, 0, 64, 0)]


def test_refusals(capi, hip):
    """every CVH_ERR_ARG / CVH_ERR_STATE of the header: the outputs stay unwritten and the contexts usable"""
    h, w = 33, 129
    L, C = capi.lib(), capi.C
    with make(capi, h, w, "rand50") as ctx, make(capi, 7, 65, "spiral", 3) as second:
        other = other_plane("grid", h, w)
        d = hip.upload(other)
        d2 = hip.upload(other_plane("grid", 7, 65))
        host_other = np.zeros((h, w), np.int32)
        bad = [(lambda: ctx.overlaps(other, 5), "conn must be 4 or 8"), (lambda: ctx.overlaps(d, 4, False, -1), "min_area must not be negative"),
               (lambda: ctx.overlaps(other, 4, False, 0, -2), "fill_holes must be -1"), (lambda: ctx.overlaps(d, 4, False, 0, 0, 2), "keep_largest must be 0 or 1"),
               (lambda: ctx.overlaps(0), "the device pointer is NULL"), (lambda: ctx.overlaps(d + 2), "is not aligned to 4 bytes"),
               (lambda: ctx.overlaps(host_other.ctypes.data), "is not device-accessible memory"),
               (lambda: capi.overlaps_batch([ctx, second], [d, 0]), "member 1: the device pointer is NULL"),
               (lambda: capi.overlaps_batch([ctx, second], [d, d2 + 1]), "member 1:"),
               (lambda: capi.overlaps_batch([ctx, second, ctx], [d, d2, d]), "member 2 duplicates member 0"),
               (lambda: capi.overlaps_batch([], []), "empty member list")]
        for call, msg in bad:
            with pytest.raises(capi.CvhError) as e:
                call()
            assert e.value.code == ERR_ARG and msg in str(e.value), (msg, str(e.value))
        table = np.full(16, 0x55, np.uint8).view(capi.OVERLAP_DTYPE)
        pairs, count = C.c_long(-9), C.c_int(-9)
        out = (C.byref(pairs), C.byref(count))
        assert L.cvh_overlaps(ctx._h, 4, 0, 0, 0, 0, None, table.ctypes.data, 1, *out) == ERR_ARG and b"other is NULL" in L.cvh_last_error(ctx._h)
        assert L.cvh_overlaps(ctx._h, 4, 0, 0, 0, 0, other.ctypes.data, table.ctypes.data, -1, *out) == ERR_ARG
        assert b"cap must not be negative" in L.cvh_last_error(ctx._h)
        assert L.cvh_overlaps_device(ctx._h, 4, 0, 0, 0, 0, d, table.ctypes.data, -1, *out, None) == ERR_ARG
        members = capi._member_array([ctx, second])
        assert L.cvh_overlaps_device_batch(members, 2, 4, 0, 0, 0, 0, None, None, None, None, None, None) == ERR_ARG
        assert b"the list of device pointers is NULL" in L.cvh_last_error(None)
        tptrs = (C.c_void_p * 2)(table.ctypes.data, None)
        assert L.cvh_overlaps_device_batch(members, 2, 4, 0, 0, 0, 0, capi._address_array([d, d2], 2), tptrs, None, None, None, None) == ERR_ARG
        assert b"tables without caps" in L.cvh_last_error(None)
        with capi.Context(8, 8, 1, capi.make_params()) as no_levelset:
            no_levelset.set_image([np.zeros((8, 8), np.uint8)])
            d3 = hip.upload(np.zeros((8, 8), np.int32))
            with pytest.raises(capi.CvhError) as e:
                no_levelset.overlaps(np.zeros((8, 8), np.int32))
            assert e.value.code == ERR_STATE and "no level set" in str(e.value)
            with pytest.raises(capi.CvhError) as e:
                capi.overlaps_batch([ctx, no_levelset], [d, d3])
            assert e.value.code == ERR_STATE and "cvh_overlaps_device_batch: member 1 has no level set" in str(e.value)
        assert (pairs.value, count.value) == (-9, -9) and (table.view(np.uint8) == 0x55).all()
        ou.assert_rows_equal(ctx.overlaps(d)[0], want_rows(ctx, other)[0])
        assert second.overlaps(d2, cap=0)[1] == want_rows(second, other_plane("grid", 7, 65))[1]
