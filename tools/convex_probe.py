#!/usr/bin/env python3
"""What does the convex relaxation buy, and what does an iteration cost on the GPU?  Records, asserts nothing.

Demonstration (--demo; the rows of tests/convex_util.py, demo_rows, on the CPU restatements, and the convex runs again on the card):
(a) the noisy disk from the checkerboard, (b) a disk whose noise is as large as its contrast, lambda scaled so that tau |r| is about
0.1, (c) the square with a thin arm of the edge-weighted row, with and without the edge plane -- iterations to the stop rule, IoU with
the clean shape and speckle of the relaxation against the level-set descent, and whether the card's mask equals the restatement's.

Cost (--cost; one process, HIP events): us per iteration -- cvh_last_run_ms of a 64-iteration cvh_convex_run without a stop rule,
"sync_every" 64, 20 timed calls after 3 -- beside cvh_geodesic_run and cvh_enqueue_steps in the per-launch flow on the same plane.
--batch: cvh_convex_run_batch against a loop of single calls (host clock), 64 x 256^2 and 8 x 1024^2.

    python tools/convex_probe.py [--demo] [--cpu-only] [--cost] [--batch] [--cases 1024x1 2048x1 4096x1 4096x3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import convex_util as X  # noqa: E402


def demo(on_card):
    rows = []
    cases = {(c[0], c[1]): c for c in X.demo_cases()}
    for r in X.demo_rows():
        row = {"probe": "convex-demo"}
        row.update({k: v for k, v in r.items() if k != "mask"})
        scene, name, img, truth, u0, gq, cset, _ = cases[(r["scene"], r["run"])]
        if on_card and cset is not None:
            from chan_vese_amd import capi
            with capi.Context(64, 64, 1, capi.make_params(mu=cset["mu"], nu=cset["nu"], lambda1=list(cset["lambda1"]), lambda2=list(cset["lambda2"]))) as c:
                c.set_image([img])
                c.set_levelset(u0)
                if gq is not None:
                    c.set_edge_map(gq)
                q = capi.make_convex_params(tau=cset["tau"], sigma=cset["sigma"], stop_rms=0.0 if scene == "a-disk" else X.DEMO_STOP,
                                            means_every=cset["means_every"], use_edge=gq is not None)
                done = capi.convex_run(c, X.DEMO_BUDGET, q)[0]
                got = c.get_mask().astype(bool)
            row["card_iterations"] = done
            row["card_mask_differs_at"] = int((got != r["mask"]).sum())
        rows.append(row)
    return rows


def cost(n, channels, reps, warmup):
    from chan_vese_amd import capi, synth
    planes = [synth.disk(n, 180 - 60 * k, 40 + 80 * k, noise=16, seed=7 + k) for k in range(channels)]
    with capi.Context(n, n, channels, capi.make_params(tol=0.0, lambda1=[1e-3] * 3, lambda2=[1e-3] * 3)) as a:
        a.set_image(planes)
        a.init_checkerboard()
        a.set_option("sync_every", 64)
        a.edge_map_from(a, 30.0)
        out = {}
        for key, use_edge in (("convex", 0), ("convex_edge", 1)):
            q = capi.make_convex_params(tau=0.25, stop_rms=-1.0, means_every=1, use_edge=use_edge)
            times = []
            for i in range(warmup + reps):
                a.init_checkerboard()
                assert capi.convex_run(a, 64, q)[0] == 64
                if i >= warmup:
                    times.append(a.last_run_ms() * 1000 / 64)
            out[key] = times
        a.init_checkerboard()
        geo, single = [], []
        for i in range(warmup + reps):
            assert capi.geodesic_run(a, 64)[0] == 64
            if i >= warmup:
                geo.append(a.last_run_ms() * 1000 / 64)
        a.set_option("resident", 0)
        a.init_checkerboard()
        for i in range(warmup + reps):
            a.enqueue_steps(64)
            a.sync()
            if i >= warmup:
                single.append(a.last_run_ms() * 1000 / 64)
    c, e, g, s = (statistics.median(x) for x in (out["convex"], out["convex_edge"], geo, single))
    px = n * n
    return {"probe": "convex-cost", "n": n, "channels": channels, "clock": "HIP events around 64 iterations", "reps": reps, "warmup": warmup,
            "convex_iteration_us": round(c, 2), "convex_min_max_us": [round(min(out["convex"]), 2), round(max(out["convex"]), 2)],
            "convex_edge_iteration_us": round(e, 2), "geodesic_iteration_us": round(g, 2), "two_phase_iteration_us": round(s, 2),
            "ratio_to_geodesic": round(c / g, 3), "ratio_to_two_phase": round(c / s, 3), "bytes_per_pixel": 64 + channels,
            "convex_gb_per_s": round((64 + channels) * px / c / 1e3, 1)}


def batch(count, n, reps, warmup):
    from chan_vese_amd import capi, synth
    planes = [synth.disk(n, 180, 40, noise=16, seed=7)]
    ctxs = [capi.Context(n, n, 1, capi.make_params(tol=0.0, lambda1=[1e-3] * 3, lambda2=[1e-3] * 3)) for _ in range(count)]
    q = capi.make_convex_params(tau=0.25, stop_rms=-1.0)
    try:
        for c in ctxs:
            c.set_image(planes)
            c.init_checkerboard()
            c.set_option("sync_every", 64)
        together, loop = [], []
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            capi.convex_run_batch(ctxs, 64, q)
            t1 = time.perf_counter()
            for c in ctxs:
                capi.convex_run(c, 64, q)
            t2 = time.perf_counter()
            if i >= warmup:
                together.append((t1 - t0) * 1e6 / 64 / count)
                loop.append((t2 - t1) * 1e6 / 64 / count)
    finally:
        for c in ctxs:
            c.close()
    b, l = statistics.median(together), statistics.median(loop)
    return {"probe": "convex-batch", "members": count, "n": n, "clock": "host clock around the calls", "reps": reps, "warmup": warmup,
            "batch_member_iteration_us": round(b, 2), "loop_member_iteration_us": round(l, 2), "speedup": round(l / b, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--demo", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--cpu-only", action="store_true", help="the demonstration on the restatements alone")
    ap.add_argument("--cases", nargs="+", default=["1024x1", "2048x1", "4096x1", "4096x3"], help="side x channels")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    if args.demo:
        rows += demo(not args.cpu_only)
    if args.cost:
        for case in args.cases:
            n, ch = (int(x) for x in case.split("x"))
            rows.append(cost(n, ch, args.reps, args.warmup))
    if args.batch:
        rows += [batch(64, 256, args.reps, args.warmup), batch(8, 1024, args.reps, args.warmup)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
