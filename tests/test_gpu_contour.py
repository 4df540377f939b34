"""Contours on the GPU (cvh_contours*) against the sequential restatement of the header's definition (contour_util).  Level sets are set
directly; every field of every loop row and every point is an integer, so EVERY comparison is ==.  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import components_util as cu
import contour_util as ct
from test_gpu_components import Hip, noisy

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = 1, 3   # cvh_status
COMBOS = [(conn, simplify) for conn in (4, 8) for simplify in (False, True)]
SMALL = ct.small_masks()


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
def noise_want():
    """the restatement of the noise plane, once: {(conn, simplify): (loops, points)}"""
    m = ct.noise()
    return m, {k: ct.trace(m, *k) for k in COMBOS}


def make(capi, mask_or_u, channels=1, **opts):
    u = np.asarray(mask_or_u)
    h, w = u.shape
    ctx = capi.Context(h, w, channels, capi.make_params(tol=0.0))
    ctx.set_option("co_resident", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_image(noisy(h, w, channels))
    ctx.set_levelset(np.where(u, 1.0, -1.0) if u.dtype == bool else u)
    return ctx


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_masks(capi, name):
    """1 x 1, rows and columns with gaps, both 2 x 2 diagonals, the checkerboard of saddles, full and empty planes, a ring with a hole and
    a blob on the border, the 64 x 64 comb (one loop of more than 4096 edges: 13 rounds of doubling); raw and inverted"""
    m = SMALL[name]
    with make(capi, m) as ctx:
        for conn, simplify in COMBOS:
            for invert in (False, True):
                want = ct.trace(m != invert, conn, simplify)
                got = ctx.contours(conn, invert, simplify=simplify)
                print(f"{name} conn {conn} simplify {simplify} invert {invert}: {got[0].size} loops, {got[1].shape[0]} points")
                ct.assert_equal(got, want, (name, conn, simplify, invert))
                assert ctx.contour_counts(conn, invert, simplify=simplify) == (want[0].size, want[1].shape[0])
    if name == "comb64":
        assert want[0].size >= 1 and int(ct.trace(m, 8)[0]["edges"][0]) > 4096 and ct.trace(m, 8)[0].size == 1
    if name == "full":
        assert ct.trace(m, 8)[0]["points"].tolist() == [4]


def test_float_state_and_special_values(capi):
    """ "state" = 32: the class comes from the float state (a positive double that rounds to 0.0f is outside); NaN, -0.0, infinities"""
    rng = np.random.default_rng(3)
    u = rng.standard_normal((37, 160)) * 3   # (a float state needs a width that is a multiple of 16, at least 144)
    flat = u.reshape(-1)
    for k, v in enumerate([np.nan, -0.0, 1e-60, -1e-60, 0.0, 1e-45, np.inf, -np.inf]):
        flat[(k * 7919 + 1) % flat.size::max(flat.size // 13, 1) + k] = v
    for state in (64, 32):
        with make(capi, u, state=state) as ctx:
            for conn, simplify in COMBOS:
                for invert in (False, True):
                    f = cu.foreground(ctx.get_levelset(), invert)
                    ct.assert_equal(ctx.contours(conn, invert, simplify=simplify), ct.trace(f, conn, simplify), (state, conn, simplify, invert))


def test_noise_plane_makes_second_trips(capi, noise_want):
    """192 x 320 seeded noise: more edges than the lanes of the member's edge sections cover in one trip, more workgroup counts than the
    one-wave scan takes in its first trip -- asserted from the library's own block functions"""
    m, want = noise_want
    raw = C.CDLL(capi.LIB_PATH)
    edges = int(want[(8, False)][0]["edges"].sum())
    pb, st, eb, el = C.c_uint(), C.c_uint(), C.c_uint(), C.c_ulonglong()
    assert raw.cvh_debug_contour_trips(m.shape[0], m.shape[1], C.c_ulonglong(edges), C.byref(pb), C.byref(st), C.byref(eb), C.byref(el)) == 0
    print(f"{edges} edges, {el.value} lanes in {eb.value} workgroups; {pb.value} pixel workgroups, {st.value} counts per scan trip")
    assert edges > el.value and pb.value > st.value
    with make(capi, m) as ctx:
        for conn, simplify in COMBOS:
            ct.assert_equal(ctx.contours(conn, simplify=simplify), want[(conn, simplify)], (conn, simplify))


def test_noise_plane_cleaned(capi, noise_want):
    """(min_area = 5, fill_holes = -1, keep_largest = 1) on the noise plane, and each step alone"""
    m, _ = noise_want
    with make(capi, m) as ctx:
        for clean in ((5, -1, True), (5, 0, False), (0, -1, False), (0, 0, True)):
            for conn, simplify in COMBOS:
                want = ct.trace_clean(m, conn, simplify, *clean)
                got = ctx.contours(conn, False, *clean, simplify=simplify)
                assert want[0].size >= 1
                ct.assert_equal(got, want, (clean, conn, simplify))
                mask = ctx.get_mask_clean(conn, False, *clean)
                ct.assert_equal(got, ct.trace(mask != 0, conn, simplify), "the mask get_mask_clean returns")


def err(capi, ctx):
    return capi.lib().cvh_last_error(ctx._h).decode()


def call(capi, ctx, loops, loop_cap, points, point_cap, conn=8, simplify=1, device=False):
    nl, npts = C.c_long(-1), C.c_long(-1)
    fn = capi.lib().cvh_contours_device if device else capi.lib().cvh_contours
    args = [ctx._h, conn, 0, 0, 0, 0, simplify, loops, loop_cap, points, point_cap, C.byref(nl), C.byref(npts)] + ([None] if device else [])
    assert fn(*args) == 0, err(capi, ctx)
    return nl.value, npts.value


def test_truncation_and_counts_only(capi, hip):
    """caps below the counts: full counts, exact prefixes, untouched bytes behind the cap -- host and device points; NULL outputs"""
    m = SMALL["ring_and_blob"]
    with make(capi, m) as ctx:
        for conn, simplify in COMBOS:
            wl, wp = ct.trace(m, conn, simplify)
            L, P = wl.size, wp.shape[0]
            assert L >= 3 and P > 8
            for lcap, pcap in ((L - 1, P - 3), (1, 1), (0, 0), (L, P), (L + 2, P + 5)):
                loops = np.full(L + 4, 0xAB, np.uint8).repeat(32).view(capi.CONTOUR_LOOP_DTYPE)
                points = np.full((P + 8, 2), 0x5A5A5A5A, np.int32)
                assert call(capi, ctx, loops.ctypes.data, lcap, points.ctypes.data, pcap, conn, int(simplify)) == (L, P)
                assert loops[:min(lcap, L)].tobytes() == wl[:min(lcap, L)].tobytes() and np.all(loops[min(lcap, L):].view(np.uint8) == 0xAB)
                assert np.array_equal(points[:min(pcap, P)], wp[:min(pcap, P)]) and np.all(points[min(pcap, P):] == 0x5A5A5A5A)
                d = hip.malloc((P + 8) * 8)
                hip.put(d, np.full((P + 8, 2), 0x5A5A5A5A, np.int32))
                loops2 = np.full(L + 4, 0xAB, np.uint8).repeat(32).view(capi.CONTOUR_LOOP_DTYPE)
                assert call(capi, ctx, loops2.ctypes.data, lcap, d, pcap, conn, int(simplify), device=True) == (L, P)
                assert loops2.tobytes() == loops.tobytes() and np.array_equal(hip.get(d, (P + 8, 2), np.int32), points)
            assert call(capi, ctx, None, 0, None, 0, conn, int(simplify)) == (L, P)
            only_loops = np.zeros(L, capi.CONTOUR_LOOP_DTYPE)
            assert call(capi, ctx, only_loops.ctypes.data, L, None, 0, conn, int(simplify)) == (L, P) and only_loops.tobytes() == wl.tobytes()
            only_points = np.zeros((P, 2), np.int32)
            assert call(capi, ctx, None, 0, only_points.ctypes.data, P, conn, int(simplify)) == (L, P) and np.array_equal(only_points, wp)
        assert capi.lib().cvh_contours(ctx._h, 8, 0, 0, 0, 0, 1, None, 0, None, 0, None, None) == 0


def test_refusals(capi, hip):
    L = capi.lib()
    with make(capi, SMALL["full"]) as ctx:
        nl, npts = C.c_long(0), C.c_long(0)
        tail = (C.byref(nl), C.byref(npts))
        for args, text in (((5, 0, 0, 0, 0, 1, None, 0, None, 0), "conn must be 4 or 8, got 5"),
                           ((8, 0, -1, 0, 0, 1, None, 0, None, 0), "min_area must not be negative"),
                           ((8, 0, 0, -2, 0, 1, None, 0, None, 0), "fill_holes must be -1"),
                           ((8, 0, 0, 0, 2, 1, None, 0, None, 0), "keep_largest must be 0 or 1, got 2"),
                           ((8, 0, 0, 0, 0, 2, None, 0, None, 0), "simplify must be 0 or 1, got 2"),
                           ((8, 0, 0, 0, 0, 1, None, -1, None, 0), "loop_cap must not be negative, got -1"),
                           ((8, 0, 0, 0, 0, 1, None, 0, None, -4), "point_cap must not be negative, got -4")):
            assert L.cvh_contours(ctx._h, *args, *tail) == ERR_ARG
            assert err(capi, ctx).startswith("cvh_contours: ") and text in err(capi, ctx), err(capi, ctx)
        d = hip.malloc(64)
        assert L.cvh_contours_device(ctx._h, 8, 0, 0, 0, 0, 1, None, 0, d + 2, 4, *tail, None) == ERR_ARG
        assert "is not aligned to 4 bytes" in err(capi, ctx)
        host = np.zeros(8, np.int32)
        assert L.cvh_contours_device(ctx._h, 8, 0, 0, 0, 0, 1, None, 0, host.ctypes.data, 4, *tail, None) == ERR_ARG
        assert "is not device-accessible memory" in err(capi, ctx)
        assert ctx.contour_counts() == (1, 4)   # the context stays usable
    with capi.Context(8, 8, 1, capi.make_params(tol=0.0)) as ctx:
        assert L.cvh_contours(ctx._h, 8, 0, 0, 0, 0, 1, None, 0, None, 0, None, None) == ERR_STATE
        assert "cvh_contours: member 0 has no level set" in err(capi, ctx)


def test_batch_of_mixed_members_equals_each_alone(capi, hip):
    """four members of mixed shapes, one and three channels (one of them empty): loops, counts and device points member by member are the
    bytes of the member called alone; a member without outputs and the cleaning options ride along"""
    masks = [ct.noise(50, 70, 1), SMALL["comb64"], SMALL["empty"], ct.noise(33, 129, 2)]
    ctxs = [make(capi, m, channels) for m, channels in zip(masks, (1, 3, 1, 3))]
    try:
        for conn, simplify in COMBOS:
            for clean in ((0, 0, False), (3, -1, False)):
                alone = [c.contours(conn, False, *clean, simplify=simplify) for c in ctxs]
                caps = [a[1].shape[0] + 2 for a in alone]
                ptrs = [hip.malloc(cap * 8) for cap in caps]
                for p, cap in zip(ptrs, caps):
                    hip.put(p, np.full((cap, 2), -7, np.int32))
                got = capi.contours_batch(ctxs, ptrs, caps, conn, False, *clean, simplify=simplify)
                for i, (nl, npts, loops) in enumerate(got):
                    assert (nl, npts) == (alone[i][0].size, alone[i][1].shape[0]) and loops.tobytes() == alone[i][0].tobytes(), (conn, simplify, clean, i)
                    pts = hip.get(ptrs[i], (caps[i], 2), np.int32)
                    assert np.array_equal(pts[:npts], alone[i][1]) and np.all(pts[npts:] == -7), (conn, simplify, clean, i)
                    ct.assert_equal(alone[i], ct.trace_clean(masks[i], conn, simplify, *clean), (conn, simplify, clean, i))
                counts = capi.contours_batch(ctxs, None, None, conn, False, *clean, simplify=simplify, loop_caps=[0, 0, 0, 0])
                assert [(c[0], c[1], c[2].size) for c in counts] == [(a[0].size, a[1].shape[0], 0) for a in alone]
    finally:
        for c in ctxs:
            c.close()


def test_a_run_continues_bit_identically(capi):
    """5 iterations continued after a call (iterations in flight, cleaned and raw) equal the run without it, bit for bit"""
    def run(with_calls, state):
        with capi.Context(96, 160, 1, capi.make_params(tol=0.0)) as ctx:
            ctx.set_option("co_resident", 0)
            ctx.set_option("state", state)
            ctx.set_image(noisy(96, 160, 1))
            ctx.init_checkerboard()
            ctx.enqueue_steps(5)
            if with_calls:
                loops, points = ctx.contours()
                assert loops.size >= 1 and points.shape[0] == int(loops["points"].sum())
                ct.assert_equal((loops, points), ct.trace(ctx.get_mask() != 0))
                ctx.contours(4, True, 4, -1, True, simplify=False)
            ctx.enqueue_steps(5)
            ctx.sync()
            return ctx.get_levelset()
    for state in (64, 32):
        assert run(True, state).tobytes() == run(False, state).tobytes()
