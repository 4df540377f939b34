"""Perona-Malik of a batch of independent contexts on one GPU: cvh_perona_malik once per context (the per-context sequence) against
cvh_perona_malik_batch (the planes of several contexts share resident launches), all in one process.  Reported in us per image-step
(an image = all of a context's channels): from the library's HIP-event intervals (cvh_last_pm_ms: summed over the sequence's calls;
the batch's one interval) and from the host's wall clock around the calls.  Every member's planes are checked byte for byte against
its own call.  Cases are COUNTxHxWxC.  EXAMPLE_A=1 also times the README's example A as a whole on EXAMPLE_A_CASE: Perona-Malik
(K=30, L=0.25, T=100) per context or batched, then cvh_run_batch for 70 iterations.
usage: pm_batch_probe.py  [CASES=64x256x256x1,32x512x512x1,8x1024x1024x1,4x2048x2048x1,16x512x512x3  K=30 L=0.25 T=100 REPS=3
                           EXAMPLE_A=1 EXAMPLE_A_CASE=64x256x256x1]"""
import os
import sys
import time

sys.path.insert(0, '.')
import numpy as np

from chan_vese_amd import capi, synth

DEFAULT = "64x256x256x1,32x512x512x1,8x1024x1024x1,4x2048x2048x1,16x512x512x3"
cases = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("CASES", DEFAULT).split(",")]
K, L, T = float(os.environ.get("K", "30")), float(os.environ.get("L", "0.25")), float(os.environ.get("T", "100"))
reps = int(os.environ.get("REPS", "3"))
steps = capi.pm_trip_count(L, T)


def make(count, h, w, ch, tol=1e-3):
    ctxs, imgs = [], []
    for b in range(count):
        ctx = capi.Context(h, w, ch, capi.make_params(tol=tol))
        r = min(h, w) // 4 + 4 * (b % 8) - 14
        img = [synth.disk(min(h, w), 200 - 20 * k, 50 + 20 * k, noise=16, seed=1000 + b + 97 * k, radius=r, h=h, w=w) for k in range(ch)]
        ctx.set_image(img)
        ctxs.append(ctx)
        imgs.append(img)
    return ctxs, imgs


def reset(ctxs, imgs):
    for ctx, img in zip(ctxs, imgs):
        ctx.set_image(img)


def per_context(ctxs):
    t0 = time.perf_counter()
    for ctx in ctxs:
        ctx.perona_malik(K, L, T)
    wall = time.perf_counter() - t0
    return sum(ctx.last_pm_ms() for ctx in ctxs), wall * 1e3


def batched(ctxs):
    t0 = time.perf_counter()
    capi.perona_malik_batch(ctxs, K, L, T)
    wall = time.perf_counter() - t0
    return ctxs[0].last_pm_ms(), wall * 1e3


print("Perona-Malik K=%g L=%g T=%g: %d steps per plane; us per image-step, median of %d (event interval / host wall clock)" % (K, L, T, steps, reps), flush=True)
for count, h, w, ch in cases:
    ctxs, imgs = make(count, h, w, ch)
    res = {}
    outs = {}
    for mode, fn in (("per-context", per_context), ("batch", batched)):
        reset(ctxs, imgs)
        fn(ctxs)                                  # warm-up (buffers, graphs, tables), untimed
        ev, wall = [], []
        for r in range(reps):
            reset(ctxs, imgs)
            e, wl = fn(ctxs)
            ev.append(e * 1e3 / (count * steps))
            wall.append(wl * 1e3 / (count * steps))
        outs[mode] = [np.stack(ctx.get_image()) for ctx in ctxs]
        info = ctxs[0].launch_info(1)
        res[mode] = (float(np.median(ev)), float(np.median(wall)))
        extra = (" batch_planes=%s batch_launches=%s" % (info.get("batch_planes"), info.get("batch_launches"))) if mode == "batch" else ""
        print("%3d x %4dx%-4d x%d  %-12s events %s median %8.3f   wall %s median %8.3f   kernel %s tiles %sx%s%s"
              % (count, h, w, ch, mode, " ".join("%.3f" % v for v in ev), res[mode][0], " ".join("%.3f" % v for v in wall), res[mode][1],
                 info["kernel"], info.get("tiles_y"), info.get("tiles_x"), extra), flush=True)
    same = all(np.array_equal(a, b) for a, b in zip(outs["per-context"], outs["batch"]))
    print("%3d x %4dx%-4d x%d  batch speed-up %.2fx (events), %.2fx (wall); planes byte-identical: %s"
          % (count, h, w, ch, res["per-context"][0] / res["batch"][0], res["per-context"][1] / res["batch"][1], same), flush=True)
    for ctx in ctxs:
        ctx.close()

if os.environ.get("EXAMPLE_A", "1") == "1":
    count, h, w, ch = (int(v) for v in os.environ.get("EXAMPLE_A_CASE", "64x256x256x1").split("x"))
    ctxs, imgs = make(count, h, w, ch)
    print("example A (-S -L 0.25 -T 100 -K 30 -N 70) on %d x %dx%d x%d: Perona-Malik, then run_batch(70); ms per batch, median of %d"
          % (count, h, w, ch, reps), flush=True)
    for mode, fn in (("per-context PM", per_context), ("batch PM", batched)):
        tot, pm_ev, run_ev = [], [], []
        for r in range(reps + 1):
            reset(ctxs, imgs)
            t0 = time.perf_counter()
            e, _ = fn(ctxs)
            for ctx in ctxs:
                ctx.init_checkerboard()
            capi.run_batch(ctxs, 70)
            wall = (time.perf_counter() - t0) * 1e3
            if r:                                 # (the first round warms up)
                tot.append(wall)
                pm_ev.append(e)
                run_ev.append(ctxs[0].last_run_ms())
        print("  %-15s wall %s median %8.2f ms   PM events median %8.2f ms   run_batch events median %7.2f ms"
              % (mode, " ".join("%.2f" % v for v in tot), float(np.median(tot)), float(np.median(pm_ev)), float(np.median(run_ev))), flush=True)
    for ctx in ctxs:
        ctx.close()
