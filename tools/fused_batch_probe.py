"""A batch of independent contexts on one GPU: wall time per image-iteration with their launches interleaved on their own streams
("resident" = 0, and the automatic flow) against the fused batch (cvh_enqueue_steps_batch: one launch per iteration for all of them),
all in one process, tol = 0, chunks of CHUNK iterations.  Cases are COUNTxHxW; STRIP_ROWS > 0 sets "strip_rows" on every context
(0: automatic -- a fused member's strips sized for its share of the chip).  The kernel printed is what ran: a context's own
instantiation, or its batch entry point (same template arguments).
usage: fused_batch_probe.py  [CASES=64x256x256,32x512x512,...  STEPS=200 CHUNK=32 REPS=3 MODES=interleaved,auto,fused STRIP_ROWS=0]"""
import os, sys, time
sys.path.insert(0, '.')
import numpy as np
from chan_vese_amd import capi, synth

DEFAULT = "64x256x256,32x512x512,16x480x640,8x1024x1024,8x1080x1920,8x2048x2048,8x4096x4096"
cases = [tuple(int(v) for v in c.split("x")) for c in os.environ.get("CASES", DEFAULT).split(",")]
steps = int(os.environ.get("STEPS", "200")); chunk = int(os.environ.get("CHUNK", "32")); reps = int(os.environ.get("REPS", "3"))
modes = os.environ.get("MODES", "interleaved,auto,fused").split(",")
strip_rows = int(os.environ.get("STRIP_ROWS", "0"))


def timed(ctxs, enqueue):
    t = []
    for r in range(reps):
        for ctx in ctxs: ctx.init_checkerboard()
        enqueue(chunk)                       # warm-up chunk (graphs, strip tables, batch tables), untimed
        for ctx in ctxs: ctx.sync()
        t0 = time.perf_counter()
        done = 0
        while done < steps:
            c = min(chunk, steps - done)
            enqueue(c)
            done += c
        for ctx in ctxs: ctx.sync()
        t.append((time.perf_counter() - t0) * 1e6 / (steps * len(ctxs)))
    return t


for count, h, w in cases:
    ctxs = []
    for b in range(count):
        ctx = capi.Context(h, w, 1, capi.make_params(tol=0.0))
        if strip_rows: ctx.set_option("strip_rows", strip_rows)
        r = min(h, w) // 4 + 4 * (b % 8) - 14
        ctx.set_image([synth.disk(min(h, w), 200, 50, noise=16, seed=1000 + b, radius=r, h=h, w=w)])
        ctx.init_checkerboard()
        ctxs.append(ctx)
    res = {}
    for mode in modes:
        if mode == "fused":
            for ctx in ctxs: ctx.set_option("resident", -1)
            t = timed(ctxs, lambda c: capi.enqueue_steps_batch(ctxs, c))
            for ctx in ctxs: ctx.set_option("resident", 0)
            kernel = ctxs[0].launch_info()["kernel"].replace("_kernel<", "_batch_kernel<", 1)
        else:
            for ctx in ctxs: ctx.set_option("resident", 0 if mode == "interleaved" else -1)

            def interleave(c):
                for ctx in ctxs: ctx.enqueue_steps(c)
            t = timed(ctxs, interleave)
            kernel = ctxs[0].launch_info()["kernel"]
        res[mode] = float(np.median(t))
        label = {"interleaved": "interleaved, resident=0", "auto": "interleaved, auto", "fused": "fused batch"}[mode]
        print("%3d x %4dx%-4d  %-24s %s  median %7.2f us per image-iteration   strip_rows %s   kernel that ran %s"
              % (count, h, w, label, " ".join("%.2f" % v for v in t), res[mode], strip_rows or "auto", kernel), flush=True)
    if "fused" in res and "interleaved" in res:
        print("%3d x %4dx%-4d  fused / interleaved (resident=0) speed-up %.2fx%s" % (count, h, w, res["interleaved"] / res["fused"],
              ("; vs auto %.2fx" % (res["auto"] / res["fused"])) if "auto" in res else ""), flush=True)
    for ctx in ctxs: ctx.close()
