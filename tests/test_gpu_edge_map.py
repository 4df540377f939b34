"""The edge plane on the card (include/chanvese_hip.h, "Edge-weighted length"): cvh_edge_map's values `==` the restatement's
(geodesic_util.py) on shapes where the replicate border and a lane's later trips can go wrong; the batch against the single calls; the
round trips of the host and device forms; refusals."""
import ctypes as C

import numpy as np
import pytest

import geodesic_util as G

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_STATE = 0, 1, 3


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def planes_of(kind, h, w, ch):
    return G.checkers(h, w, ch) if kind == "checkers" else G.random_planes(h, w, ch)


def context(capi, planes):
    h, w = planes[0].shape
    ctx = capi.Context(h, w, len(planes), capi.make_params(tol=0.0))
    ctx.set_image(planes)
    return ctx


@pytest.mark.parametrize("kind", ["random", "checkers"])
@pytest.mark.parametrize("shape", G.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_map_equals_the_restatement(capi, shape, kind):
    h, w, ch = shape
    planes = planes_of(kind, h, w, ch)
    ctx = context(capi, planes)
    try:
        for K in G.EDGE_KS:
            ctx.edge_map_from(ctx, K)
            got, want = ctx.get_edge_map(), G.edge_map(planes, K)
            assert got.dtype == np.uint16 and np.array_equal(got, want), (K, np.argwhere(got != want)[:5])
        assert all(np.array_equal(a, b) for a, b in zip(ctx.get_image(), planes))   # src is only read
    finally:
        ctx.close()


def test_three_channels_into_one_and_the_batch(capi):
    """a 3-channel source into a 1-channel destination (C is the source's); every shape in ONE call equals its single call byte for
    byte; a source may serve two destinations and be a destination itself"""
    srcs, dsts, singles, Ks = [], [], [], []
    try:
        for i, (h, w, ch) in enumerate(G.EDGE_SHAPES):
            for kind in ("random", "checkers"):
                s = context(capi, planes_of(kind, h, w, ch))
                srcs.append(s)
                dsts.append(s if kind == "random" else capi.Context(h, w, 1, capi.make_params()))
                Ks.append(G.EDGE_KS[i % 3])
        three = context(capi, planes_of("random", 67, 65, 3))
        one = capi.Context(67, 65, 1, capi.make_params())
        srcs += [three, three]
        dsts += [one, capi.Context(67, 65, 3, capi.make_params())]
        Ks += [30.0, 0.5]
        one.edge_map_from(three, 30.0)
        assert np.array_equal(one.get_edge_map(), G.edge_map(three.get_image(), 30.0))
        for s, d, K in zip(srcs, dsts, Ks):
            d.edge_map_from(s, K)
            singles.append(d.get_edge_map())
            d.set_edge_map(np.zeros((d.h, d.w), dtype=np.uint16))
        capi.edge_map_batch(dsts, srcs, Ks)
        for s, d, K, single in zip(srcs, dsts, Ks, singles):
            got = d.get_edge_map()
            assert np.array_equal(got, single) and np.array_equal(got, G.edge_map(s.get_image(), K))
    finally:
        for c in set(srcs + dsts):
            c.close()


def test_round_trips(capi):
    from test_gpu_device_io import Hip
    hip = Hip()
    h, w = 9, 70
    rng = np.random.default_rng(3)
    gq = rng.integers(0, G.ONE + 1, (h, w)).astype(np.uint16)
    gq[0, 0], gq[-1, -1] = 0, G.ONE
    ctx = capi.Context(h, w, 1, capi.make_params())
    try:
        L = capi.lib()
        out = np.zeros((h, w), dtype=np.uint16)
        assert L.cvh_get_edge_map(ctx._h, out.ctypes.data) == ERR_STATE and "no edge plane" in L.cvh_last_error(ctx._h).decode()
        ctx.set_edge_map(gq)
        assert np.array_equal(ctx.get_edge_map(), gq)
        over = gq.copy()
        over[3, 5] = G.ONE + 1
        assert L.cvh_set_edge_map(ctx._h, over.ctypes.data) == ERR_ARG and "value 32769 at pixel" in L.cvh_last_error(ctx._h).decode()
        assert np.array_equal(ctx.get_edge_map(), gq)                         # nothing was touched
        # the device forms: the range check is a clamp
        wild = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        d_in, d_out = hip.upload(wild, offset=2), hip.malloc(wild.nbytes + 2) + 2
        ctx.set_edge_map(d_in)
        assert np.array_equal(ctx.get_edge_map(), np.minimum(wild, G.ONE))
        ctx.get_edge_map(ptr=d_out)
        assert np.array_equal(hip.get(d_out, (h, w), np.uint16), np.minimum(wild, G.ONE))
        assert L.cvh_set_edge_map_device(ctx._h, d_in + 1, None) == ERR_ARG and "not aligned" in L.cvh_last_error(ctx._h).decode()
        assert L.cvh_set_edge_map_device(ctx._h, wild.ctypes.data, None) == ERR_ARG and "not device-accessible" in L.cvh_last_error(ctx._h).decode()
        assert L.cvh_get_edge_map_device(ctx._h, None, None) == ERR_ARG
        # the image and level-set calls do not touch the plane
        ctx.set_image([rng.integers(0, 256, (h, w), dtype=np.uint8)])
        ctx.init_checkerboard()
        ctx.run(2)
        assert np.array_equal(ctx.get_edge_map(), np.minimum(wild, G.ONE))
        hip.free_all()
    finally:
        ctx.close()


def test_refusals(capi):
    L = capi.lib()
    err = lambda: L.cvh_last_error(None).decode()
    planes = G.random_planes(8, 20, 1)
    a, other, empty = context(capi, planes), context(capi, G.random_planes(8, 21, 1)), capi.Context(8, 20, 1, capi.make_params())
    try:
        a.edge_map_from(a, 30.0)
        before = a.get_edge_map()
        for K, text in ((0.0, "K = 0"), (-2.0, "K = -2"), (float("nan"), "K = nan"), (float("inf"), "K = inf"), (1e200, "K = 1e+200")):
            assert L.cvh_edge_map(a._h, a._h, K) == ERR_ARG and text in err(), err()
        assert L.cvh_edge_map(a._h, other._h, 30.0) == ERR_ARG and "must be 8 x 21 too" in err()
        assert L.cvh_edge_map(a._h, empty._h, 30.0) == ERR_STATE and "the source context has no image" in err()
        assert L.cvh_edge_map(a._h, None, 30.0) == ERR_ARG and "the source context is NULL" in err()
        two = (C.c_void_p * 2)(a._h.value, a._h.value)
        ks = (C.c_double * 2)(30.0, 30.0)
        assert L.cvh_edge_map_batch(two, two, 2, ks) == ERR_ARG and "a destination may be listed once" in err()
        assert L.cvh_edge_map_batch(two, two, 2, None) == ERR_ARG and "K is NULL" in err()
        assert np.array_equal(a.get_edge_map(), before)
        empty.edge_map_from(a, 30.0)                                          # a destination needs no image
        assert np.array_equal(empty.get_edge_map(), before)
    finally:
        for c in (a, other, empty):
            c.close()
