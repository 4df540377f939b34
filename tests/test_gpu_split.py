"""Object split on the card (include/chanvese_hip.h, "Object split") against the restatement (split_util.py): labels, table, count, the
cut and the baked level set with ==, at the shapes of the kernels' seams -- a single row, a single column, 2 x 2, one tile of the growth,
one row and one column past it, two tiles each way, a width that is no multiple of a 16-byte piece --; both connectivities, invert,
cleaning; the demonstration scene; a spiral corridor that takes more sweeps than a group holds; a member alone against the same member
inside a batch; that cvh_split only reads; that cvh_split_levelset leaves the components of F0 \\ cut; two calls in a row.
Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import components_util as CU
import morph_util as M
import split_util as S
from test_gpu_device_io import Hip

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 3
bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


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


@pytest.fixture(scope="module")
def geometry(capi):
    return capi.split_geometry()


def sweeps(capi):
    fn = capi.lib().cvh_debug_split_sweeps
    fn.restype = C.c_ulong
    return fn()


def context_of(capi, u, channels=1, with_image=False, **options):
    h, w = u.shape
    ctx = capi.Context(h, w, channels, capi.make_params(tol=0.0))
    for k, v in options.items():
        ctx.set_option(k, v)
    if with_image:
        ctx.set_image(M.planes_of(h, w, channels))
    ctx.set_levelset(u)
    return ctx


def check(capi, hip, ctx, want, tag, **kw):
    """labels, table and count of cvh_split, then the level set of cvh_split_levelset (and with it the cut), against `want`"""
    h, w = want.f0.shape
    d_lab = hip.malloc(h * w * 4 + 64)
    hip.put(d_lab, np.full(h * w + 16, -7, np.int32))
    _, table, k = ctx.split(labels_ptr=d_lab, cap=want.K + 3, **kw)
    got = hip.get(d_lab, (h * w + 16,), np.int32)
    assert k == want.K, (tag, k, want.K)
    assert np.array_equal(got[:h * w].reshape(h, w), want.labels), (tag, int((got[:h * w].reshape(h, w) != want.labels).sum()))
    assert (got[h * w:] == -7).all(), tag                              # nothing behind the plane is written
    assert np.array_equal(table, want.table), (tag, table, want.table)
    assert ctx.split(cap=0, **kw)[2] == want.K                          # counts alone
    ctx.split_levelset(inside=2.5, outside=-0.125, **kw)
    u = ctx.get_levelset()
    assert np.array_equal(bits(u), bits(np.where(want.pieces, 2.5, -0.125))), (tag, int((bits(u) != bits(np.where(want.pieces, 2.5, -0.125))).sum()))
    cut = (want.labels > 0) & (ctx.get_mask() == 0)
    assert np.array_equal(cut, want.cut), tag


# ---- 1. every output at the small shapes and the tile seams ----
@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("name", list(S.CASES))
def test_small_planes(capi, hip, name, conn):
    for h, w in S.SMALL_SHAPES:
        for r2 in (0, 1, 4):
            with context_of(capi, S.case(name, h, w)) as ctx:
                check(capi, hip, ctx, S.expected(name, h, w, conn, r2), (name, (h, w), conn, r2), r2=r2, conn=conn)


@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("which", range(5))
def test_tile_seams(capi, hip, geometry, which, conn):
    h, w = S.shapes(*geometry[:2])[which]
    assert which != 4 or (w % 4 and (h * w) % 4)                        # no multiple of the 16-byte piece of int32 labels
    for name in ("touching", "all_inside", "all_outside"):
        for r2 in ((0, 9, 25) if name == "touching" else (4,)):
            with context_of(capi, S.case(name, h, w), channels=3 if which == 3 else 1) as ctx:
                check(capi, hip, ctx, S.expected(name, h, w, conn, r2), (name, (h, w), conn, r2), r2=r2, conn=conn)


# ---- 2. the parameters of the start set ----
@pytest.mark.parametrize("conn", (4, 8))
def test_invert_and_cleaning(capi, hip, conn):
    h, w = 40, 70
    for name, invert, clean in (("noisy", True, (0, 0, False)), ("noisy", False, (6, -1, False)), ("touching", False, (3, 5, True)),
                                ("touching", True, (2, 0, False))):
        want = S.expected(name, h, w, conn, 4, invert, clean)
        with context_of(capi, S.case(name, h, w)) as ctx:
            check(capi, hip, ctx, want, (name, conn, invert, clean), r2=4, conn=conn, invert=invert, min_area=clean[0], fill_holes=clean[1],
                  keep_largest=clean[2])


def test_float_state(capi, hip):
    want = S.expected("touching", 40, 144, 4, 9)                        # (the float state needs a width that is a multiple of 16 and >= 144)
    with context_of(capi, S.case("touching", 40, 144), state=32) as ctx:
        check(capi, hip, ctx, want, "state 32", r2=9)


# ---- 3. the demonstration ----
def test_the_demonstration(capi, hip):
    d = S.demonstration()
    for r2, k, areas in ((81, 4, [9, 423, 406, 60]), (100, 4, [9, 416, 413, 60]), (49, 3, [9, 829, 60]), (150, 3, [9, 829, 60]), (64, 5, None)):
        want = S.Split(d, 4, r2)
        with context_of(capi, M.levelset_of(d)) as ctx:
            _, table, got_k = ctx.split(r2=r2, cap=8)
            assert got_k == k and (areas is None or table["area"].tolist() == areas), (r2, got_k, table)
            check(capi, hip, ctx, want, ("demonstration", r2), r2=r2)


# ---- 4. more sweeps than a group: a corridor through every seam of a two-by-two-tile plane ----
def test_the_spiral_takes_more_sweeps_than_a_group(capi, hip, geometry):
    tr, tc, group = geometry
    m, centre = S.spiral(2 * tr, 2 * tc)
    want = S.Split(m, 4, 1)
    assert want.K == 1 and want.markers[centre]
    with context_of(capi, M.levelset_of(m)) as ctx:
        before = sweeps(capi)
        assert ctx.split(r2=1, cap=0)[2] == 1
        ran = sweeps(capi) - before
        print("sweeps", ran, "group", group)
        assert ran > group, (ran, group)
        check(capi, hip, ctx, want, "spiral", r2=1)
    with context_of(capi, M.levelset_of(m)) as ctx:
        check(capi, hip, ctx, S.Split(m, 8, 1), "spiral conn 8", r2=1, conn=8)


# ---- 5. a member alone and inside a batch; two calls in a row ----
def test_a_batch_of_mixed_members_equals_each_member_alone(capi, hip, geometry):
    tr, tc, _ = geometry
    members = [("touching", tr + 5, tc + 7, 1, 9), ("demo", 64, 64, 3, 81), ("noisy", 7, 1, 1, 1), ("all_outside", 9, 21, 3, 4), ("touching", 2 * tr, 2 * tc, 1, 25)]
    ctxs = [context_of(capi, S.case(name, h, w), c) for name, h, w, c, _ in members]
    try:
        r2 = [m[4] for m in members]
        ptrs = [hip.malloc(h * w * 4) for _, h, w, _, _ in members]
        ptrs[3] = 0                                                     # a member without a label plane
        for rep in range(2):                                            # two calls in a row: the same bytes
            counts = capi.split_batch(ctxs, ptrs, r2=r2, conn=4)
            for (name, h, w, _, r), p, k in zip(members, ptrs, counts):
                want = S.expected(name, h, w, 4, r)
                assert k == want.K, (name, rep)
                if p:
                    assert np.array_equal(hip.get(p, (h, w), np.int32), want.labels), (name, rep)
        assert capi.split_batch(ctxs, None, r2=r2) == counts
        capi.split_levelset_batch(ctxs, r2=r2, inside=1.0, outside=-1.0)
        for (name, h, w, _, r), ctx in zip(members, ctxs):
            want = S.expected(name, h, w, 4, r)
            assert np.array_equal(bits(ctx.get_levelset()), bits(np.where(want.pieces, 1.0, -1.0))), name
    finally:
        for c in ctxs:
            c.close()


# ---- 6. cvh_split only reads; cvh_split_levelset leaves the components of F0 \ cut ----
def test_a_run_continued_after_split_is_bit_identical(capi, hip):
    h, w = 48, 80
    u0 = np.where(S.CASES["touching"](h, w), 1.0, -1.0)
    outs = []
    for with_split in (False, True):
        with context_of(capi, u0, with_image=True) as ctx:
            ctx.run(6)
            if with_split:
                d_lab = hip.malloc(h * w * 4)
                ctx.split(r2=9, labels_ptr=d_lab, cap=None)
            ctx.run(6)
            outs.append(ctx.get_levelset())
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.parametrize("conn", (4, 8))
def test_components_after_split_levelset(capi, hip, conn):
    h, w = 64, 64
    want = S.expected("demo", h, w, 4, 81)
    with context_of(capi, S.case("demo", h, w)) as ctx:
        ctx.split_levelset(r2=81, conn=4)
        d_lab = hip.malloc(h * w * 4)
        k, table = ctx.components(conn=conn, labels_ptr=d_lab, cap=16)
        lab, tab = CU.label(want.pieces, conn)
        assert k == tab.size == 4 and np.array_equal(table, tab) and np.array_equal(hip.get(d_lab, (h, w), np.int32), lab)
        ctx.split_levelset(r2=0, conn=conn)                            # a second split of the pieces at r2 = 0 changes nothing
        assert np.array_equal(ctx.get_mask().astype(bool), want.pieces)


# ---- 7. refusals ----
def test_refusals(capi, hip):
    L = capi.lib()
    with context_of(capi, S.case("noisy", 9, 21)) as ctx, capi.Context(9, 21) as empty:
        d_lab = hip.malloc(9 * 21 * 4 + 8)
        for kw in (dict(conn=5), dict(min_area=-1), dict(fill_holes=-2), dict(keep_largest=2)):
            with pytest.raises(capi.CvhError):
                ctx.split(r2=1, **kw)
        with pytest.raises(capi.CvhError) as e:
            ctx.split(r2=1, labels_ptr=d_lab + 2)
        assert "not aligned to 4 bytes" in str(e.value)
        with pytest.raises(capi.CvhError) as e:
            capi.split_batch([ctx, empty], r2=1)
        assert "member 1 has no level set" in str(e.value)
        with pytest.raises(capi.CvhError):
            capi.split_levelset_batch([ctx, ctx], r2=1)
        with context_of(capi, S.case("noisy", 7, 1)) as other:         # the refusals name the member: a bad pointer of member 1
            host = np.zeros(16, np.int32)
            for bad, text in ((d_lab + 2, "member 1: "), (host.ctypes.data, "member 1: ")):
                with pytest.raises(capi.CvhError) as e:
                    capi.split_batch([ctx, other], [d_lab, bad], r2=1)
                assert "cvh_split_batch" in str(e.value) and text in str(e.value) and ("not aligned to 4 bytes" in str(e.value) or "not device-accessible" in str(e.value)), str(e.value)
        assert L.cvh_split_batch(capi._member_array([ctx]), 1, 4, 0, 0, 0, 0, None, None, None, None) == ERR_ARG
        assert ctx.split(r2=1, cap=0)[2] == S.expected("noisy", 9, 21, 4, 1).K   # and the context stays usable
