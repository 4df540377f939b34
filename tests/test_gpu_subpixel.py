"""Subpixel contours on the GPU (cvh_contours_subpixel*) against the restatement of the header's definition (subpixel_util).  Level sets
are set directly; every bit of a point is defined, so EVERY comparison is ==.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import contour_util as ct
import subpixel_util as su
from test_gpu_components import Hip, noisy

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = 1, 3   # cvh_status
COMBOS = [(conn, invert) for conn in (4, 8) for invert in (False, True)]
SMALL = dict(ct.small_masks(), **{"1x9_full": np.ones((1, 9), bool), "9x1_full": np.ones((9, 1), bool)})
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


@pytest.fixture
def hip(capi):
    h = Hip()
    yield h
    h.free_all()


@pytest.fixture(scope="module")
def noise_u():
    return su.from_mask(ct.noise(), seed=21)


def make(capi, u, channels=1, **opts):
    u = np.asarray(u, dtype=np.float64)
    h, w = u.shape
    ctx = capi.Context(h, w, channels, capi.make_params(tol=0.0))
    ctx.set_option("co_resident", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_image(noisy(h, w, channels))
    ctx.set_levelset(u)
    return ctx


def assert_equal(got, want, what=""):
    """every field of every loop row, and every point bit for bit (no NaN can occur: == on the doubles, and the bytes)"""
    (gl, gp), (wl, wp) = got, want
    assert gl.size == wl.size, (what, gl.size, wl.size)
    for f in ct.LOOP_DTYPE.names:
        assert np.array_equal(gl[f], wl[f]), (what, f, gl[f][:8], wl[f][:8])
    assert gp.shape == wp.shape and gp.dtype == np.float64, (what, gp.shape, wp.shape)
    bad = np.nonzero((gp != wp).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:8], gp[bad[:8]], wp[bad[:8]])
    assert gp.tobytes() == np.ascontiguousarray(wp).tobytes(), what


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_masks(capi, name):
    """1 x 1, 1 x N and N x 1 (with gaps and full: every edge of an end pixel is a plane-border edge), both diagonals, the checkerboard,
    a plane wholly inside, an empty one, ring and blob, the comb: random magnitudes, raw and inverted; the loop rows are
    cvh_contours(simplify = 0)'s.  The integer call runs first: its point table is the one the subpixel call must outgrow."""
    m = SMALL[name]
    u = su.from_mask(m, seed=len(name))
    with make(capi, u) as ctx:
        for conn, invert in COMBOS:
            want = su.trace_subpixel(u, conn, invert)
            rows = ctx.contours(conn, invert, simplify=False)[0]
            got = ctx.contours_subpixel(conn, invert)
            print(f"{name} conn {conn} invert {invert}: {got[0].size} loops, {got[1].shape[0]} points")
            assert_equal(got, want, (name, conn, invert))
            assert got[0].tobytes() == rows.tobytes()
    if name == "full":
        assert want[1].shape[0] == 0 and su.trace_subpixel(u, 8)[1].shape[0] == 2 * (13 + 21)


@pytest.mark.parametrize("state", [64, 32])
def test_special_values(capi, state):
    """NaN, +-0.0, +-1e-50 (0.0f as a float: background, and with "state" = 32 a zero), +-inf, +-1e308 neighbours whose difference
    overflows (with "state" = 32 they are infinities): the midpoint wherever the header says so"""
    u = su.special()
    with make(capi, u, state=state) as ctx:
        held = ctx.get_levelset()
        assert np.array_equal(held, su.as_state(u, state == 32), equal_nan=True)
        for conn, invert in COMBOS:
            want = su.trace_subpixel(u, conn, invert, state32=state == 32)
            assert_equal(ctx.contours_subpixel(conn, invert), want, (state, conn, invert))
            assert np.all(np.isfinite(want[1]))
    _, pts, ids = su.trace_subpixel_edges(u, 8, state32=state == 32)
    assert pts[ids.tolist().index(4 * (5 * u.shape[1] + 20) + 1)].tolist() == [21.0, 5.5]   # the overflowing (or infinite) pair


def test_noise_plane_raw_and_cleaned(capi, noise_u):
    """192 x 320 seeded noise with random magnitudes: lanes of the edge sections make second trips (asserted from the library's own
    block function); raw, and cleaned with (min_area, fill_holes, keep_largest)"""
    raw = C.CDLL(capi.LIB_PATH)
    with make(capi, noise_u) as ctx:
        for clean in ((0, 0, False), (5, -1, True), (3, 0, False)):
            for conn, invert in COMBOS:
                want = su.trace_subpixel(noise_u, conn, invert, *clean)
                assert_equal(ctx.contours_subpixel(conn, invert, *clean), want, (clean, conn, invert))
                if clean == (0, 0, False):
                    pb, st, eb, el = C.c_uint(), C.c_uint(), C.c_uint(), C.c_ulonglong()
                    assert raw.cvh_debug_contour_trips(192, 320, C.c_ulonglong(want[1].shape[0]), C.byref(pb), C.byref(st), C.byref(eb), C.byref(el)) == 0
                    assert want[1].shape[0] > el.value


def err(capi, ctx):
    return capi.lib().cvh_last_error(ctx._h).decode()


def call(capi, ctx, loops, loop_cap, points, point_cap, conn=8, device=False):
    nl, npts = C.c_long(-1), C.c_long(-1)
    fn = capi.lib().cvh_contours_subpixel_device if device else capi.lib().cvh_contours_subpixel
    args = [ctx._h, conn, 0, 0, 0, 0, loops, loop_cap, points, point_cap, C.byref(nl), C.byref(npts)] + ([None] if device else [])
    assert fn(*args) == 0, err(capi, ctx)
    return nl.value, npts.value


def test_truncation_and_counts_only(capi, hip):
    """caps below the counts: full counts, exact prefixes, nothing written behind the cap (a sentinel fill) -- host and device points;
    NULL outputs; loop_cap = 0"""
    u = su.from_mask(SMALL["ring_and_blob"], 8)
    with make(capi, u) as ctx:
        for conn in (4, 8):
            wl, wp = su.trace_subpixel(u, conn)
            L, P = wl.size, wp.shape[0]
            assert L >= 3 and P > 8
            for lcap, pcap in ((L - 1, P - 3), (1, 1), (0, 0), (0, P), (L, P), (L + 2, P + 5)):
                loops = np.full(L + 4, 0xAB, np.uint8).repeat(32).view(capi.CONTOUR_LOOP_DTYPE)
                points = np.full((P + 8, 2), SENTINEL)
                assert call(capi, ctx, loops.ctypes.data, lcap, points.ctypes.data, pcap, conn) == (L, P)
                assert loops[:min(lcap, L)].tobytes() == wl[:min(lcap, L)].tobytes() and np.all(loops[min(lcap, L):].view(np.uint8) == 0xAB)
                assert np.array_equal(points[:min(pcap, P)], wp[:min(pcap, P)]) and np.all(points[min(pcap, P):] == SENTINEL)
                d = hip.malloc((P + 8) * 16)
                hip.put(d, np.full((P + 8, 2), SENTINEL))
                loops2 = np.full(L + 4, 0xAB, np.uint8).repeat(32).view(capi.CONTOUR_LOOP_DTYPE)
                assert call(capi, ctx, loops2.ctypes.data, lcap, d, pcap, conn, device=True) == (L, P)
                assert loops2.tobytes() == loops.tobytes() and np.array_equal(hip.get(d, (P + 8, 2), np.float64), points)
            d = hip.malloc((P + 1) * 16)   # a device array that is 8-byte but not 16-byte aligned
            hip.put(d, np.full((P + 1, 2), SENTINEL))
            assert call(capi, ctx, None, 0, d + 8, P, conn, device=True) == (L, P)
            flat = hip.get(d, (2 * P + 2,), np.float64)
            assert flat[0] == SENTINEL and flat[-1] == SENTINEL and np.array_equal(flat[1:-1].reshape(P, 2), wp)
            assert call(capi, ctx, None, 0, None, 0, conn) == (L, P)
            only_loops = np.zeros(L, capi.CONTOUR_LOOP_DTYPE)
            assert call(capi, ctx, only_loops.ctypes.data, L, None, 0, conn) == (L, P) and only_loops.tobytes() == wl.tobytes()
            only_points = np.zeros((P, 2))
            assert call(capi, ctx, None, 0, only_points.ctypes.data, P, conn) == (L, P) and np.array_equal(only_points, wp)
        assert capi.lib().cvh_contours_subpixel(ctx._h, 8, 0, 0, 0, 0, None, 0, None, 0, None, None) == 0


def test_refusals(capi, hip):
    L = capi.lib()
    with make(capi, su.from_mask(SMALL["full"], 1)) as ctx:
        nl, npts = C.c_long(0), C.c_long(0)
        tail = (C.byref(nl), C.byref(npts))
        for args, text in (((5, 0, 0, 0, 0, None, 0, None, 0), "conn must be 4 or 8, got 5"),
                           ((8, 0, -1, 0, 0, None, 0, None, 0), "min_area must not be negative"),
                           ((8, 0, 0, -2, 0, None, 0, None, 0), "fill_holes must be -1"),
                           ((8, 0, 0, 0, 2, None, 0, None, 0), "keep_largest must be 0 or 1, got 2"),
                           ((8, 0, 0, 0, 0, None, -1, None, 0), "loop_cap must not be negative, got -1"),
                           ((8, 0, 0, 0, 0, None, 0, None, -4), "point_cap must not be negative, got -4")):
            assert L.cvh_contours_subpixel(ctx._h, *args, *tail) == ERR_ARG
            assert err(capi, ctx).startswith("cvh_contours_subpixel: ") and text in err(capi, ctx), err(capi, ctx)
        d = hip.malloc(256)
        assert L.cvh_contours_subpixel_device(ctx._h, 8, 0, 0, 0, 0, None, 0, d + 4, 4, *tail, None) == ERR_ARG
        assert err(capi, ctx).startswith("cvh_contours_subpixel_device: ") and "is not aligned to 8 bytes" in err(capi, ctx)
        host = np.zeros(16)
        assert L.cvh_contours_subpixel_device(ctx._h, 8, 0, 0, 0, 0, None, 0, host.ctypes.data, 4, *tail, None) == ERR_ARG
        assert "is not device-accessible memory" in err(capi, ctx)
        members = (C.c_void_p * 2)(ctx._h, ctx._h)
        assert L.cvh_contours_subpixel_device_batch(members, 2, 8, 0, 0, 0, 0, None, None, None, None, None, None, None) == ERR_ARG
        assert "cvh_contours_subpixel_device_batch: member 1 duplicates member 0" in err(capi, ctx), err(capi, ctx)
        pts = (C.c_void_p * 1)(d)
        single = (C.c_void_p * 1)(ctx._h)
        assert L.cvh_contours_subpixel_device_batch(single, 1, 8, 0, 0, 0, 0, None, None, pts, None, None, None, None) == ERR_ARG
        assert "point arrays without point_caps" in err(capi, ctx)
        loops, points = ctx.contours_subpixel()   # the context stays usable
        assert loops.size == 1 and points.shape == (2 * (13 + 21), 2)
    with capi.Context(8, 8, 1, capi.make_params(tol=0.0)) as ctx:
        assert L.cvh_contours_subpixel(ctx._h, 8, 0, 0, 0, 0, None, 0, None, 0, None, None) == ERR_STATE
        assert "cvh_contours_subpixel: member 0 has no level set" in err(capi, ctx)


def test_batch_of_mixed_members_equals_each_alone(capi, hip):
    """five members of mixed shapes, one and three channels -- an empty mask, a float-state member, a member without a point array --:
    loops, counts and device points member by member are the bytes of the member called alone, cleaning options included"""
    us = [su.from_mask(ct.noise(50, 70, 1), 1), su.from_mask(SMALL["comb64"], 2), su.from_mask(SMALL["empty"], 3),
          su.from_mask(ct.noise(33, 129, 2), 4), su.special()]
    ctxs = [make(capi, u, channels, **opts) for u, channels, opts in zip(us, (1, 3, 1, 3, 1), ({}, {}, {}, {}, {"state": 32}))]
    try:
        for conn, invert in COMBOS:
            for clean in ((0, 0, False), (3, -1, False)):
                alone = [c.contours_subpixel(conn, invert, *clean) for c in ctxs]
                for i, u in enumerate(us):
                    assert_equal(alone[i], su.trace_subpixel(u, conn, invert, *clean, state32=i == 4), (conn, invert, clean, i))
                caps = [a[1].shape[0] + 2 for a in alone]
                ptrs = [hip.malloc(cap * 16) for cap in caps]
                for p, cap in zip(ptrs, caps):
                    hip.put(p, np.full((cap, 2), SENTINEL))
                ptrs[1] = 0   # no point array for the comb
                got = capi.contours_subpixel_batch(ctxs, ptrs, caps, conn, invert, *clean)
                for i, (nl, npts, loops) in enumerate(got):
                    assert (nl, npts) == (alone[i][0].size, alone[i][1].shape[0]) and loops.tobytes() == alone[i][0].tobytes(), (conn, invert, clean, i)
                    if not ptrs[i]:
                        continue
                    pts = hip.get(ptrs[i], (caps[i], 2), np.float64)
                    assert pts[:npts].tobytes() == alone[i][1].tobytes() and np.all(pts[npts:] == SENTINEL), (conn, invert, clean, i)
                assert (got[2][0], got[2][1]) == ((0, 0) if not invert else (1, 2 * (13 + 21)))
                counts = capi.contours_subpixel_batch(ctxs, None, None, conn, invert, *clean, loop_caps=[0] * 5)
                assert [(c[0], c[1], c[2].size) for c in counts] == [(a[0].size, a[1].shape[0], 0) for a in alone]
    finally:
        for c in ctxs:
            c.close()


def test_after_reinit_every_point_is_a_midpoint(capi):
    """the distance to a pixel-edge front: a = 0.5, b = -0.5 on every edge"""
    u = su.from_mask(SMALL["ring_and_blob"], 5)
    with make(capi, u) as ctx:
        before = ctx.contours_subpixel(8)
        ctx.reinit()
        loops, pts = ctx.contours_subpixel(8)
        assert_equal((loops, pts), (before[0], su.midpoints(u, 8)), "reinit")
        assert np.any(before[1] != pts)
        assert np.array_equal(pts * 2, np.round(pts * 2))


def test_a_run_continues_bit_identically(capi):
    """5 iterations continued after a call (iterations in flight, cleaned and raw) equal the run without it, bit for bit; the points
    taken with iterations in flight are the restatement's for the level set a settled twin holds"""
    def run(with_calls, state):
        with capi.Context(96, 160, 1, capi.make_params(tol=0.0)) as ctx:
            ctx.set_option("co_resident", 0)
            ctx.set_option("state", state)
            ctx.set_image(noisy(96, 160, 1))
            ctx.init_checkerboard()
            ctx.enqueue_steps(5)
            got = None
            if with_calls:
                got = ctx.contours_subpixel()
                ctx.contours_subpixel(4, True, 4, -1, True)
            else:
                ctx.sync()
                got = su.trace_subpixel(ctx.get_levelset())
            ctx.enqueue_steps(5)
            ctx.sync()
            return ctx.get_levelset(), got
    for state in (64, 32):
        (u1, got), (u0, want) = run(True, state), run(False, state)
        assert u1.tobytes() == u0.tobytes()
        assert got[0].size >= 1
        assert_equal(got, want, state)


def test_disk_64_device_points_lie_on_the_circle(capi):
    """the analytic disk of the issue: the device's points within 0.01 px of the circle (the restatement gives 0.0056), the lattice
    loop's midpoints not within 0.4"""
    u = su.disk(64)
    with make(capi, u) as ctx:
        loops, pts = ctx.contours_subpixel(8)
        lattice = ctx.contours(8, simplify=False)[1]
    sub = su.radial_error(pts)
    mids = (lattice + np.roll(lattice, -1, axis=0)) / 2.0   # (one loop: consecutive lattice points are an edge's ends)
    print(f"{pts.shape[0]} edges: subpixel {sub:.4f} px, midpoints {su.radial_error(mids):.4f} px")
    assert loops.size == 1 and pts.shape[0] == 162
    assert sub <= 0.01
    assert su.radial_error(mids) >= 0.4
    assert_equal((loops, pts), su.trace_subpixel(u, 8), "disk")
