"""cvh_convex_run_batch on the card: members of mixed shapes, channel counts, parameters and math modes in two orders -- every member
bit for bit its own single run, every member stopping on its own."""
import numpy as np
import pytest

import convex_util as X
from test_gpu_convex import bits, capi, cp, make   # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu

# (shape, set, mode, use_edge, stop_rms): the last two stop early, at different iterations
MEMBERS = [((24, 64, 1), "A", "strict", 0, -1.0), ((67, 65, 3), "B", "fast", 1, -1.0), ((X.M.SEAM_H, 130, 1), "B", "strict", 1, -1.0),
           ((8, 4096, 1), "A", "fast", 1, -1.0), ((67, 65, 3), "A", "strict", 0, 0.0975), ((9, 122, 1), "B", "fast", 0, 0.1), ((1, 7, 1), "A", "fast", 0, -1.0)]
STEPS = 8


def build(capi, m):
    shape, which, mode, edge, stop = m
    planes, u, gq = X.case_inputs(*shape)
    return make(capi, planes, u, gq, X.SETS[which], mode), cp(capi, X.SETS[which], use_edge=edge, stop_rms=stop)


def results(ctx, r):
    return (r[0], bits(r[1]), bits(r[2]), bits(ctx.get_levelset())) + tuple(bits(a) for a in ctx.relaxed(duals=True))


@pytest.fixture(scope="module")
def singles(capi):
    out = []
    for m in MEMBERS:
        ctx, q = build(capi, m)
        try:
            out.append(results(ctx, capi.convex_run(ctx, STEPS, q, trace=True)))
        finally:
            ctx.close()
    return out


@pytest.mark.parametrize("order", [list(range(len(MEMBERS))), [5, 1, 6, 0, 4, 3, 2]], ids=["as-listed", "shuffled"])
def test_every_member_is_its_single_run(capi, singles, order):
    built = [build(capi, MEMBERS[i]) for i in order]
    ctxs = [c for c, _ in built]
    try:
        res = capi.convex_run_batch(ctxs, STEPS, [q for _, q in built], trace=True)
        got = [results(c, r) for c, r in zip(ctxs, res)]
        # a resumed batch goes on where the members' own single resumed runs go on
        more = capi.convex_run_batch(ctxs[:2], 3, [cp(capi, X.SETS[MEMBERS[i][1]], use_edge=MEMBERS[i][3], resume=1) for i in order[:2]])
        assert [r[0] for r in more] == [3, 3]
    finally:
        for c in ctxs:
            c.close()
    steps = [g[0] for g in got]
    print("steps", dict(zip(order, steps)))
    for i, g in zip(order, got):
        want = singles[i]
        assert g[0] == want[0], i
        for x, y in zip(g[1:], want[1:]):
            assert np.array_equal(x, y), i
    by_member = dict(zip(order, steps))
    assert by_member[0] == STEPS and 1 <= by_member[4] < STEPS and 1 <= by_member[5] < STEPS   # members stop on their own


def test_a_batch_of_one_is_the_single_call(capi, singles):
    ctx, q = build(capi, MEMBERS[1])
    try:
        got = results(ctx, capi.convex_run_batch([ctx], STEPS, q, trace=True)[0])
    finally:
        ctx.close()
    assert got[0] == singles[1][0] and all(np.array_equal(x, y) for x, y in zip(got[1:], singles[1][1:]))
