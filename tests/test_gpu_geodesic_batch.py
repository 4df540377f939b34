"""cvh_geodesic_run_batch on the card: a member is bit for bit its own single run -- level set, steps, norm and trace -- for a mix of
shapes, channel counts, modes and parameters, one member stopping early, in any member order; a batch of one is the single call."""
import numpy as np
import pytest

import geodesic_util as G
from test_gpu_geodesic import MODES, bits, make

pytestmark = pytest.mark.gpu

# (h, w, channels, parameter set, edge plane, mode); the last one stops early (the stop case's tol)
MEMBERS = [(67, 65, 3, "other", "random", "fast"), (24, 64, 1, "default", "sobel", "strict"), (8, 4096, 1, "default", "random", "fast"),
           (G.M.SEAM_H, 130, 1, "other", "random", "strict"), (67, 65, 3, "default", "sobel", "strict"), (1, 7, 1, "other", "random", "fast"),
           G.STOP_SHAPE + ("stop", "random", "fast")]
STEPS = 8


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def member(capi, spec):
    h, w, ch, which, kind, mode = spec
    planes, u, gq = G.case_inputs(h, w, ch, kind)
    p = dict(G.DEFAULT, tol=G.stop_case()[0]) if which == "stop" else G.params_of(which)
    return make(capi, planes, u, gq, p, mode)


@pytest.fixture(scope="module")
def singles(capi):
    out = []
    for spec in MEMBERS:
        ctx = member(capi, spec)
        try:
            steps, norm, trace = capi.geodesic_run(ctx, STEPS, trace=True)
            out.append((steps, norm, trace, ctx.get_levelset()))
        finally:
            ctx.close()
    assert out[-1][0] == G.stop_case()[1] < STEPS and all(s[0] == STEPS for s in out[:-1])
    return out


@pytest.mark.parametrize("order", [list(range(len(MEMBERS))), [6, 2, 4, 0, 5, 3, 1]], ids=["in-order", "shuffled"])
def test_a_member_is_its_own_run(capi, singles, order):
    ctxs = [member(capi, MEMBERS[i]) for i in order]
    try:
        res = capi.geodesic_run_batch(ctxs, STEPS, trace=True)
        for i, ctx, (steps, norm, trace) in zip(order, ctxs, res):
            s = singles[i]
            assert steps == s[0] and norm == s[1], MEMBERS[i]
            assert np.array_equal(bits(trace), bits(s[2])) and np.array_equal(bits(ctx.get_levelset()), bits(s[3])), MEMBERS[i]
            assert ctx.sync()[0] == 0
    finally:
        for c in ctxs:
            c.close()


def test_a_batch_of_one_is_the_single_call(capi, singles):
    ctx = member(capi, MEMBERS[0])
    try:
        (steps, norm, trace), = capi.geodesic_run_batch([ctx], STEPS, trace=True)
        s = singles[0]
        assert steps == s[0] and norm == s[1] and np.array_equal(bits(trace), bits(s[2]))
        assert np.array_equal(bits(ctx.get_levelset()), bits(s[3]))
    finally:
        ctx.close()
