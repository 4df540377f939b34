#!/usr/bin/env python3
"""What a reinitialisation costs on the GPU, beside one CSV iteration of the same plane (one fresh process; run on an MI355X).

us per cvh_reinit from HIP events inside the library (cvh_debug_last_reinit_ms: table copy, the three launches, flag copy), median of
`--reps` calls after two warm-up calls, at 256^2 .. 4096^2, for two inputs scaled to size: the BASELINE disk's level set after 50
iterations (distances up to n / 4: the row pass's worst case) and a noisy disk's after 20.  Beside each: us of one CSV iteration of that
plane (cvh_last_run_ms over 64 enqueued iterations) and their ratio; the row pass's trip counts per pixel, counted on the host from the
level set (min(vertical distance to the other class, columns to the farther edge) is the kernel's upper bound, the search stops
earlier at k^2 >= best); and cvh_reinit_batch over 64 x 256^2 against 64 single calls.  Bytes per pixel are counted from the shapes.

  python tools/reinit_probe.py --out profiles/r09_reinit/reinit_probe.txt
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from chan_vese_amd import capi, synth  # noqa: E402


def reinit_ms(ctx):
    v = ctypes.c_float(0)
    fn = ctypes.CDLL(capi.LIB_PATH).cvh_debug_last_reinit_ms
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
    assert fn(ctx._h, ctypes.byref(v)) == 0
    return v.value


def trip_bound(u, every=1):
    """mean / max over the pixels of every `every`-th row of the row pass's upper bound on trips: min(vertical distance to the other
    class, max(j, w - 1 - j)).  The column pass runs on the full mask; rows are sampled behind it."""
    import reinit_util as R
    m = R.mask_of(u)
    g0, g1 = R.column_pass(m)
    g = np.where(m, g0, g1)[::every]
    w = u.shape[1]
    edge = np.maximum(np.arange(w), w - 1 - np.arange(w))[None, :]
    t = np.minimum(g, edge)
    return float(t.mean()), int(t.max())


def measure(n, case, reps, out):
    planes, steps = ([synth.disk(n)], 50) if case == "disk" else ([synth.disk(n, 200, 50, noise=48, seed=77)], 20)
    with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image(planes)
        ctx.init_checkerboard()
        ctx.run(steps)
        u = ctx.get_levelset()
        times = []
        for r in range(reps + 2):
            ctx.set_levelset(u)                       # the same input every time (a reinitialised level set has the same mask anyway)
            assert ctx.reinit()
            if r >= 2:
                times.append(1e3 * reinit_ms(ctx))
        ctx.set_levelset(u)
        ctx.enqueue_steps(64); ctx.sync()           # warm: graph build
        ctx.enqueue_steps(64); ctx.sync()
        it_us = 1e3 * ctx.last_run_ms() / 64
    mean_t, max_t = trip_bound(u, 1 if n <= 2048 else 8)
    t = float(np.median(times))
    print(f"{n:5d}^2 {case:6s} reinit {t:9.1f} us (min {min(times):.1f}, max {max(times):.1f}; {reps} calls)   CSV iteration {it_us:7.1f} us"
          f"   = {t / it_us:6.1f} iterations   trip bound per pixel: mean {mean_t:.1f}, max {max_t}", file=out, flush=True)


def batch(reps, out):
    n, m = 256, 64
    ctxs = []
    for i in range(m):
        c = capi.Context(n, n, 1, capi.make_params(tol=0.0))
        c.set_image([synth.disk(n, 200, 50, noise=32, seed=i)])
        c.init_checkerboard()
        ctxs.append(c)
    capi.run_batch(ctxs, 20)
    us = [c.get_levelset() for c in ctxs]
    one, fused, wall_one, wall_fused = [], [], [], []
    for r in range(reps + 2):
        for c, u in zip(ctxs, us):
            c.set_levelset(u)
        t0 = time.perf_counter()
        dev = 0.0
        for c in ctxs:
            c.reinit()
            dev += reinit_ms(c)
        t1 = time.perf_counter()
        for c, u in zip(ctxs, us):
            c.set_levelset(u)
        t2 = time.perf_counter()
        capi.reinit_batch(ctxs)
        t3 = time.perf_counter()
        if r >= 2:
            one.append(1e3 * dev); fused.append(1e3 * reinit_ms(ctxs[0])); wall_one.append(1e6 * (t1 - t0)); wall_fused.append(1e6 * (t3 - t2))
    for c in ctxs:
        c.close()
    print(f"64 x 256^2: 64 single calls {np.median(one):.1f} us of device intervals, {np.median(wall_one):.1f} us of host time; "
          f"one cvh_reinit_batch {np.median(fused):.1f} us device, {np.median(wall_fused):.1f} us host", file=out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[256, 1024, 2048, 4096])
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    print(f"{capi.lib().cvh_version().decode()}; bytes per pixel moved by the three launches: 8 (u) + 0.125 + 0.125 (class words) + 4 + 4 "
          "(distance fields) + 8 (u') = 24.25, floor 16", file=out)
    for n in a.sizes:
        for case in ("disk", "noisy"):
            measure(n, case, a.reps, out)
    batch(a.reps, out)


if __name__ == "__main__":
    main()
