"""The three marching-wave flows behind ONE leader on the card: a context leads a geodesic batch of 3 members, then a localised batch of
2 (radius 2 and 5), then is A of the first of 2 four-phase pairs, with cvh_localized_means and cvh_multiphase_means in between.  The
leader's table and pinned block are reused with three record sizes, three slot strides and shrinking member counts; every member's
level set, steps, norm and trace -- and both means calls -- are bit for bit those of the same call made with fresh contexts.  Shapes:
24 x 64 x 1 and 67 x 65 x 3 (a partial wave-column and a partial strip), 4 iterations, FAST and STRICT members in every batch."""
import numpy as np
import pytest

import geodesic_util as G
import multiphase_util as M
from test_gpu_geodesic import bits, make

pytestmark = pytest.mark.gpu
STEPS = 4
BIG, SMALL = (67, 65, 3), (24, 64, 1)
RADII = (2, 5)
RUNS = ("geodesic", "localized", "multiphase")


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def sequence(capi, reuse):
    """the five calls in order.  reuse: ONE context is the first member of every call, its level set put back to the case's in front of
    each; else every call is made with fresh contexts.  {call: its members' (level set, steps, norms, trace), or the means}"""
    made = []

    def new(shape, mode, p, second=False):
        planes, u1, gq = G.case_inputs(*shape, "random")
        made.append(make(capi, planes, M.case_inputs(*shape)[2] if second else u1, gq, p, mode))
        return made[-1]

    def first():
        if not reuse or not made:
            return new(BIG, "fast", M.OTHER_A)
        made[0].set_levelset(G.case_inputs(*BIG, "random")[1])
        return made[0]

    out = {}
    try:
        ctxs = [first(), new(SMALL, "strict", M.DEFAULT), new(BIG, "strict", M.DEFAULT)]
        out["geodesic"] = [(c.get_levelset(), r[0], np.array(r[1]), r[2]) for c, r in zip(ctxs, capi.geodesic_run_batch(ctxs, STEPS, trace=True))]
        out["localized_means"] = first().localized_means(RADII[0])
        ctxs = [first(), new(SMALL, "strict", M.DEFAULT)]
        out["localized"] = [(c.get_levelset(), r[0], np.array(r[1]), r[2]) for c, r in zip(ctxs, capi.localized_run_batch(ctxs, RADII, STEPS, trace=True))]
        out["multiphase_means"] = capi.multiphase_means(first(), new(BIG, "fast", M.OTHER_B, second=True))
        pairs = [(first(), new(BIG, "fast", M.OTHER_B, second=True)), (new(SMALL, "strict", M.DEFAULT), new(SMALL, "strict", M.DEFAULT, second=True))]
        out["multiphase"] = [(np.stack([a.get_levelset(), b.get_levelset()]), r[0], np.array(r[1]), r[2])
                             for (a, b), r in zip(pairs, capi.multiphase_run_batch(pairs, STEPS, trace=True))]
    finally:
        for c in made:
            c.close()
    return out


def test_one_leader_through_the_three_flows(capi):
    want, got = sequence(capi, reuse=False), sequence(capi, reuse=True)
    assert [len(want[k]) for k in RUNS] == [3, 2, 2]
    for k in RUNS:
        for i, (g, w) in enumerate(zip(got[k], want[k])):
            assert g[1] == w[1] == STEPS and w[3].shape[0] == STEPS, (k, i, g[1], w[1])
            for name, x, y in zip(("level set", "norm", "trace"), (g[0], g[2], g[3]), (w[0], w[2], w[3])):
                assert x.shape == y.shape and np.array_equal(bits(x), bits(y)), (k, i, name)
            assert np.isfinite(w[3]).all() and (w[2] > 0).all(), (k, i, "the reference ran")
    for key in ("c1", "c2", "wq", "a", "s"):
        x, y = got["localized_means"][key], want["localized_means"][key]
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint64), y.view(np.uint64)), key
    assert np.array_equal(bits(got["multiphase_means"]), bits(want["multiphase_means"]))
