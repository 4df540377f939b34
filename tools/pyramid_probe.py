#!/usr/bin/env python3
"""What does a coarse-to-fine run cost and buy on the GPU?  Records, asserts nothing.
 (a) us per cvh_restrict_image and per cvh_prolong_levelset call (host clock around `reps` calls, each call ends in its one host wait)
     at 4096^2 -> 2048^2 and 2048^2 -> 1024^2, beside the us of one CSV iteration of the fine plane in the same process
     (cvh_last_run_ms of a 64-iteration enqueue, the second of two);
 (b) noisy disks (chan_vese_amd.synth.disk, noise 32, default parameters, tol 1e-3, checkerboard start) at 1024^2, 2048^2, 4096^2 and
     4096^2 x 3: device time (the sum of cvh_last_run_ms over the levels) and iterations per level of a 3-level pyramid against the
     one-level run from the same kind of start, and the polarity-agnostic IoU of the two final masks.  The restrict / prolong calls of the
     pyramid are timed with the host clock and listed apart.
Prints one JSON line per case and writes them to --out.

    python tools/pyramid_probe.py [--sizes 1024 2048 4096] [--levels 3] [--reps 20] [--max-steps 4000] [--out pyramid_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chan_vese_amd import capi, synth  # noqa: E402


def iou_either(a, b):
    a, b = a.astype(bool), b.astype(bool)
    best = 0.0
    for cand in (b, ~b):
        union = (a | cand).sum()
        best = max(best, float((a & cand).sum()) / float(union) if union else 1.0)
    return best


def per_call_us(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def calls(n, reps):
    img = synth.disk(n, noise=32, seed=3)
    with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as fine, capi.Context(n // 2, n // 2, 1) as coarse:
        coarse.set_option("co_resident", 0)
        fine.set_image([img])
        fine.init_checkerboard()
        coarse.init_checkerboard()
        for _ in range(2):
            fine.enqueue_steps(64)
            fine.sync()
        row = {"probe": "calls", "fine": n, "coarse": n // 2, "csv_iteration_us": round(fine.last_run_ms() * 1000 / 64, 2),
               "restrict_us": round(per_call_us(lambda: fine.restrict_image_to(coarse), reps), 1),
               "prolong_us": round(per_call_us(lambda: coarse.prolong_levelset_to(fine), reps), 1), "reps": reps}
    return row


def pyramid(n, channels, levels, max_steps):
    planes = [synth.disk(n, 200 - 30 * k, 50 + 20 * k, noise=32, seed=3 + k) for k in range(channels)]
    row = {"probe": "pyramid", "n": n, "channels": channels, "levels": levels}
    with capi.Context(n, n, channels) as ctx:
        ctx.set_image(planes)
        ctx.init_checkerboard()
        done, _ = ctx.run(max_steps)
        single = ctx.get_mask()
        row["one_level"] = {"iterations": int(done), "stopped": bool(ctx.sync()[2]), "run_ms": round(ctx.last_run_ms(), 3)}
    ctxs = [capi.Context(h, w, channels) for h, w in capi.pyramid_shapes(n, n, levels)]
    try:
        ctxs[0].set_image(planes)
        ctxs[-1].init_checkerboard()
        t0 = time.perf_counter()
        for k in range(levels - 1):
            ctxs[k].restrict_image_to(ctxs[k + 1])
        down_ms = (time.perf_counter() - t0) * 1e3
        ctxs[-1].init_checkerboard()
        t0 = time.perf_counter()
        res = capi.run_coarse_to_fine(ctxs, max_steps)
        wall_ms = (time.perf_counter() - t0) * 1e3
        run_ms = [c.last_run_ms() for c in ctxs]
        row["pyramid"] = {"iterations": [int(r[0]) for r in res], "run_ms": [round(v, 3) for v in run_ms], "run_ms_total": round(sum(run_ms), 3),
                          "restrict_chain_host_ms": round(down_ms, 3), "driver_host_ms": round(wall_ms, 3),
                          "iou_with_one_level": round(iou_either(single, ctxs[0].get_mask()), 6)}
    finally:
        for c in ctxs:
            c.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-steps", type=int, default=4000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []

    def record(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for n in (4096, 2048):
        record(calls(n, args.reps))
    for n in args.sizes:
        record(pyramid(n, 1, args.levels, args.max_steps))
    if 4096 in args.sizes:
        record(pyramid(4096, 3, args.levels, args.max_steps))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
