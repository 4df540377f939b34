#!/usr/bin/env python3
"""What does the edge-weighted length term do, and what does an iteration cost on the GPU?  Records, asserts nothing.

Demonstration (--demo; the CPU restatement's runs of tests/geodesic_util.py, demo_runs, and the same runs on the card): a 64 x 64 noisy
square with a thin arm, Otsu start, plain Chan-Vese at mu = 0.5 / 5 / 20 / 100 and the edge-weighted runs at the smallest speckle-free
mu and above, the map built from the Perona-Malik-smoothed plane: IoU with the clean shape, speckle components, share of the arm kept,
and whether the card's mask equals the restatement's on every pixel.

Cost (--cost; one process, HIP events): us per iteration -- cvh_last_run_ms of a 64-iteration cvh_geodesic_run with tol = 0 and
"sync_every" 64, 20 timed calls after 3 -- beside cvh_enqueue_steps in the per-launch flow and one four-phase pair-iteration on the same
plane, and cvh_edge_map with the host clock.  --batch: cvh_geodesic_run_batch against a loop of single calls.

    python tools/geodesic_probe.py [--demo] [--cost] [--batch] [--cases 1024x1 2048x1 4096x1 4096x3] [--out FILE]
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

import geodesic_util as G  # noqa: E402


def demo(on_card):
    runs, best = G.demo_runs()
    img, shape, arm = G.demo_scene()
    u0, t = G.demo_start(img)
    rows = []
    for name, (m, iou, speckle, kept, firm) in runs.items():
        row = {"probe": "geodesic-demo", "run": name, "otsu": t, "best_plain_mu": best, "steps": G.demo_steps(float(name.split("mu=")[1].split()[0])), "dt": G.demo_dt(float(name.split("mu=")[1].split()[0])), "iou": round(iou, 4), "speckle": speckle,
               "arm_kept": round(kept, 3)}
        if on_card:
            from chan_vese_amd import capi
            mu = float(name.split("mu=")[1].split()[0])
            p = G.demo_params(mu)
            with capi.Context(64, 64, 1, capi.make_params(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in p.items()})) as c:
                c.set_image([img])
                c.set_levelset(u0)
                if name.startswith("edge"):
                    K, L, T = G.DEMO_PM
                    with capi.Context(64, 64, 1, capi.make_params()) as s:
                        s.set_image([img])
                        s.perona_malik(K, L, T)
                        row["smoothed_equals_cpu"] = bool(np.array_equal(s.get_image()[0], G.demo_smoothed(img)))
                        c.edge_map_from(s, float(name.split("K=")[1]))
                else:
                    c.set_edge_map(np.full((64, 64), G.ONE, dtype=np.uint16))
                capi.geodesic_run(c, G.demo_steps(mu))
                got = c.get_mask()
            row["card_mask_equals_cpu"] = bool(np.array_equal(got, m))
            row["card_mask_differs_at"] = int((got != m).sum())
            row["restatement_pixels_not_firm"] = int((~firm).sum())
            row["card_mask_differs_at_firm_pixels"] = int(((got != m) & firm).sum())
        rows.append(row)
    return rows


def cost(n, channels, reps, warmup):
    from chan_vese_amd import capi, synth
    planes = [synth.disk(n, 180 - 60 * k, 40 + 80 * k, noise=16, seed=7 + k) for k in range(channels)]
    mk = lambda: capi.Context(n, n, channels, capi.make_params(tol=0.0))
    with mk() as a, mk() as b:
        for ctx in (a, b):
            ctx.set_image(planes)
            ctx.init_checkerboard()
        b.set_levelset(np.roll(a.get_levelset(), (2, 3), axis=(0, 1)))
        a.set_option("sync_every", 64)
        edge = []
        for i in range(warmup + 5):
            t0 = time.perf_counter()
            a.edge_map_from(a, 30.0)
            if i >= warmup:
                edge.append((time.perf_counter() - t0) * 1e6)
        geo, pair, single = [], [], []
        for i in range(warmup + reps):
            assert capi.geodesic_run(a, 64)[0] == 64
            if i >= warmup:
                geo.append(a.last_run_ms() * 1000 / 64)
        a.init_checkerboard()
        for i in range(warmup + reps):
            assert capi.multiphase_run(a, b, 64)[0] == 64
            if i >= warmup:
                pair.append(a.last_run_ms() * 1000 / 64)
        a.set_option("resident", 0)
        a.init_checkerboard()
        for i in range(warmup + reps):
            a.enqueue_steps(64)
            a.sync()
            if i >= warmup:
                single.append(a.last_run_ms() * 1000 / 64)
    g, p, s = statistics.median(geo), statistics.median(pair), statistics.median(single)
    return {"probe": "geodesic-cost", "n": n, "channels": channels, "clock": "HIP events around 64 iterations", "reps": reps, "warmup": warmup,
            "geodesic_iteration_us": round(g, 2), "geodesic_min_max_us": [round(min(geo), 2), round(max(geo), 2)],
            "four_phase_pair_iteration_us": round(p, 2), "two_phase_iteration_us": round(s, 2),
            "ratio_to_pair": round(g / p, 3), "ratio_to_two_phase": round(g / s, 3), "edge_map_host_clock_us": round(statistics.median(edge), 1),
            "bytes_per_pixel": 18 + channels}


def batch(count, n, reps, warmup):
    from chan_vese_amd import capi, synth
    planes = [synth.disk(n, 180, 40, noise=16, seed=7)]
    ctxs = [capi.Context(n, n, 1, capi.make_params(tol=0.0)) for _ in range(count)]
    try:
        for c in ctxs:
            c.set_image(planes)
            c.init_checkerboard()
            c.edge_map_from(c, 30.0)
            c.set_option("sync_every", 64)
        together, loop = [], []
        for i in range(warmup + reps):
            t0 = time.perf_counter()
            capi.geodesic_run_batch(ctxs, 64)
            t1 = time.perf_counter()
            for c in ctxs:
                capi.geodesic_run(c, 64)
            t2 = time.perf_counter()
            if i >= warmup:
                together.append((t1 - t0) * 1e6 / 64 / count)
                loop.append((t2 - t1) * 1e6 / 64 / count)
    finally:
        for c in ctxs:
            c.close()
    b, l = statistics.median(together), statistics.median(loop)
    return {"probe": "geodesic-batch", "members": count, "n": n, "clock": "host clock around the calls", "reps": reps, "warmup": warmup,
            "batch_member_iteration_us": round(b, 2), "loop_member_iteration_us": round(l, 2), "speedup": round(l / b, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--demo", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--cpu-only", action="store_true", help="the demonstration on the restatement alone")
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
