"""Helpers of the fused-batch GPU tests (test_gpu_fused_batch.py, test_gpu_fused_batch_matrix.py): members, initial level sets, the
two reference bars (bits of the member's own run, the oracle with the member's own parameters) and the host arithmetic of a member's
share geometry (csv_batch.hip batch_share, csv_run.hip resolve_geometry)."""
import ctypes as C

import numpy as np

from chan_vese_amd import synth

STRICT, FAST = 1, 2
KBATCH_OWN_ROWS = 32      # csv_batch.hip, kBatchOwnRows: members whose own strips have this many rows keep their own geometry


def planes(h, w, ch, seed, noise=16):
    n = min(h, w)
    if ch == 1:
        return [synth.disk(n, 200, 50, noise=noise, seed=seed, h=h, w=w)]
    return [synth.disk(n, fg, bg, noise=noise, seed=seed + k, h=h, w=w) for k, (fg, bg) in enumerate([(180, 40), (200, 60), (60, 200)])]


def cone(h, w):
    """A smooth initial level set (its norms fall monotonically after the first iterations, unlike the checkerboard's)."""
    ii = np.arange(h)[:, None] - h / 2 + 37
    jj = np.arange(w)[None, :] - w / 2 - 21
    return (min(h, w) / 3 - np.sqrt(ii * ii + jj * jj)) / 4.0


def member(capi, h, w, ch=1, opts=None, seed=0, tol=0.0, trace=64, **pk):
    ctx = capi.Context(h, w, ch, capi.make_params(tol=tol, **pk))
    for k, v in (opts or {}).items():
        ctx.set_option(k, v)
    ctx.set_option("trace", trace)
    ctx.set_image(planes(h, w, ch, seed))
    return ctx


def result(ctx, steps):
    done, nrm, stopped = ctx.sync()
    return ctx.get_levelset().tobytes(), ctx.get_trace(steps), done, stopped


def assert_same(a, b, what):
    assert a[2] == b[2] and a[3] == b[3], (what, a[2:], b[2:])
    assert a[1].shape == b[1].shape and a[1].tobytes() == b[1].tobytes(), (what, np.abs(a[1] - b[1]).max())
    assert a[0] == b[0], what


def iou(a, b):
    return (a & b).sum() / max((a | b).sum(), 1)


def tol_for_stop(capi, ctx, k, steps, pk):
    """tol at which the member's stop rule fires at iteration k: from its own tol = 0 run's norm trace."""
    ctx.set_params(capi.make_params(tol=1.0, **pk))
    ctx.set_levelset(cone(ctx.h, ctx.w))
    scale = ctx.get_stop_condition()          # ||mean_k I_k||_2 (tol = 1)
    ctx.set_params(capi.make_params(tol=0.0, **pk))
    ctx.set_levelset(cone(ctx.h, ctx.w))
    ctx.run(steps)
    norms = ctx.get_trace(steps)[:, -1]
    tol = norms[k - 1] / scale * (1 + 1e-6)
    assert norms[:k - 1].min() > norms[k - 1] * (1 + 1e-5), "the norm of iteration k must be the first below the threshold"
    return tol


def first_stop_at_or_after(norms, k):
    """The first iteration >= k whose norm is below every earlier one by 1e-5 (a tol set just above it stops the run there)."""
    for j in range(max(k, 2), len(norms) + 1):
        if norms[:j - 1].min() > norms[j - 1] * (1 + 1e-5):
            return j
    raise AssertionError(f"no clean stop iteration at or after {k}")


def assert_oracle(oracle, ctx, imgs, u0, pk, steps, what, done=None):
    """The oracle bar: csv_run with the member's OWN parameters and image; level set <= 1e-9 max|u|, every trace row rtol 1e-9, mask
    exact, steps_done and the stop iteration equal."""
    u_c, done_c, _, tr_c = oracle.csv_run(imgs, u0, oracle.make_params(**pk), steps)
    s = ctx.sync()
    assert s[0] == done_c and (s[2] or done_c == steps), (what, s, done_c)
    if done is not None:
        assert done == done_c, (what, done, done_c)
    u_g = ctx.get_levelset()
    err = np.abs(u_g - u_c).max() / np.abs(u_c).max()
    assert err <= 1e-9, (what, err)
    tr_g = ctx.get_trace(done_c)
    assert tr_g.shape == tr_c.shape and np.allclose(tr_g, tr_c, rtol=1e-9, atol=0), (what, np.abs(tr_g - tr_c).max())
    assert np.array_equal(ctx.get_mask(), oracle.mask(u_c)), what
    return done_c


# ---- host arithmetic of the share geometry (csv_batch.hip): batch_share, then resolve_geometry with the share as the CU count ----

def num_cus(capi, ctx):
    out = C.c_int(0)
    fn = capi.lib().cvh_debug_num_cus
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    assert fn(ctx._h, C.byref(out)) == 0
    return out.value


def share(cus, n_i, n_tot):
    """batch_share: round(num_cus x n_i / sum n), at least 1 CU."""
    return max(1, int(cus * n_i / n_tot + 0.5))


def data_flow(capi, h, w, channels=1, math_mode=0, kernel=-1, state=64, cus=256):
    """resolve_geometry for the default options and `cus` CUs: (kernel 2 | 3, wave-columns, strips, strip rows, workgroups)."""
    fn = capi.lib().cvh_debug_data_flow
    out = [C.c_int(0) for _ in range(4)]
    assert fn(h, w, channels, math_mode, kernel, state, cus, *[C.byref(o) for o in out]) == 0
    flow, tx, ty, sr = (o.value for o in out)
    nblocks = ((tx + 3) // 4) * ty if flow == 2 else ((tx + 1) // 2) * ((ty + 1) // 2)
    return flow, tx, ty, sr, nblocks


def last_grid(capi, ctx):
    """Workgroups (bookkeeper excluded) of the last per-launch wave launch the context took part in, own or fused."""
    buf = (C.c_ulonglong * 1)()
    words, nblocks = C.c_long(0), C.c_int(0)
    fn = capi.lib().cvh_debug_read
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_int)]
    assert fn(ctx._h, buf, 0, C.byref(words), C.byref(nblocks)) == 0
    return nblocks.value
