#!/usr/bin/env python3
"""What does the four-phase model do, and what does an iteration of a pair cost on the GPU?  Records, asserts nothing.

Demonstration (--demo; CPU restatement of tests/multiphase_util.py, and the card where there is one): a 64 x 64 image, two level sets
from the checkerboard and its (2, 3) roll, default parameters, run to the stop rule (tol 1e-3) or --max-steps: the iterations, the four
means, the share of pixels with the right class after the best of the 24 relabellings, and the two-phase result beside it.  Images:
"disks" -- two overlapping disks, grey levels 40 / 100 / 160 / 220 on their four regions -- and "nested" -- three nested squares, 40 / 100 /
160 / 220 from the outside in.

Cost (--cost; one process, HIP events): us per pair iteration -- cvh_last_run_ms of a 64-iteration cvh_multiphase_run with tol = 0
and "sync_every" 64, 20 timed calls after 3 -- beside TWO iterations of cvh_enqueue_steps of the same plane in the per-launch flow
("resident" 0; 64-iteration enqueues, the same counts), and their ratio.

    python tools/multiphase_probe.py --demo [--noise 4] [--max-steps 400] [--cost] [--cases 1024x1 2048x1 4096x1 4096x3] [--out FILE]
"""
import argparse
import itertools
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import multiphase_util as M  # noqa: E402
import np_restatement as R  # noqa: E402


def nested_image(n, noise, seed=11):
    yy, xx = np.mgrid[0:n, 0:n]
    d = np.maximum(np.abs(xx - (n - 1) / 2), np.abs(yy - (n - 1) / 2)) / (n / 2)
    cls = (d < 0.8).astype(int) + (d < 0.55).astype(int) + (d < 0.3).astype(int)
    g = np.array(M.LEVELS, dtype=np.float64)[cls] + np.random.default_rng(seed).normal(0.0, noise, (n, n))
    return [np.clip(np.rint(g), 0, 255).astype(np.uint8)], cls


def best_relabelling(labels, cls):
    return max(float((np.array(p)[labels] == cls).mean()) for p in itertools.permutations(range(4)))


def two_phase(planes, u, p, max_steps):
    stop = R.stop_condition(planes, p["tol"])
    for t in range(max_steps):
        u, nrm, c1, c2 = R.csv_step(planes, u, p["mu"], p["nu"], p["dt"], p["eps"])
        if nrm <= stop:
            return t + 1, c1[0], c2[0]
    return max_steps, c1[0], c2[0]


def demo(image, noise, max_steps, on_card):
    n = 64
    planes, cls = M.disks_image(n, n, 1, noise) if image == "disks" else nested_image(n, noise)
    u1, u2 = M.starts(n, n)
    p = dict(M.DEFAULT, tol=1e-3)
    v1, v2, steps, trace = M.run(planes, u1, u2, p, p, max_steps)
    c = M.means(planes, v1, v2)
    row = {"probe": "multiphase-demo", "image": image, "n": n, "noise": noise, "starts": "checkerboard, checkerboard rolled (2, 3)",
           "params": "mu 0.5 nu 0 dt 1 eps 1 tol 1e-3 lambda 1", "max_steps": max_steps,
           "cpu": {"steps": steps, "stopped": steps < max_steps, "means_11_10_01_00": [round(float(x), 2) for x in c[:, 0]],
                   "right_class_share": round(best_relabelling(M.labels(v1, v2), cls), 4)}}
    s2, c1, c2 = two_phase(planes, u1, p, max_steps)
    row["two_phase_cpu"] = {"steps": s2, "means": [round(c1, 2), round(c2, 2)]}
    if on_card:
        from chan_vese_amd import capi
        mk = lambda: capi.Context(n, n, 1, capi.make_params(tol=1e-3))
        with mk() as a, mk() as b:
            for ctx, u in ((a, u1), (b, u2)):
                ctx.set_image(planes)
                ctx.set_levelset(u)
            gsteps, norms, _ = capi.multiphase_run(a, b, max_steps)
            lab = a.multiphase_labels_with(b)
            row["card"] = {"steps": gsteps, "means_11_10_01_00": [round(float(x), 2) for x in capi.multiphase_means(a, b)[:, 0]],
                           "right_class_share": round(best_relabelling(lab, cls), 4),
                           "labels_equal_cpu_share": round(float((lab == M.labels(v1, v2)).mean()), 4)}
    return row


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
        pair = []
        for i in range(warmup + reps):
            assert capi.multiphase_run(a, b, 64)[0] == 64
            if i >= warmup:
                pair.append(a.last_run_ms() * 1000 / 64)
        a.set_option("resident", 0)
        a.init_checkerboard()
        single = []
        for i in range(warmup + reps):
            a.enqueue_steps(64)
            a.sync()
            if i >= warmup:
                single.append(a.last_run_ms() * 1000 / 64)
        kernel = a.launch_info()["kernel"]
    p, s = statistics.median(pair), statistics.median(single)
    return {"probe": "multiphase-cost", "n": n, "channels": channels, "clock": "HIP events around 64 iterations", "reps": reps, "warmup": warmup,
            "pair_iteration_us": round(p, 2), "pair_min_max_us": [round(min(pair), 2), round(max(pair), 2)],
            "two_phase_iteration_us": round(s, 2), "two_phase_kernel": kernel.split("<")[0],
            "ratio_pair_to_two_two_phase": round(p / (2 * s), 3), "bytes_per_pixel": [32 + channels, 2 * (16 + channels)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--demo", action="store_true")
    ap.add_argument("--cost", action="store_true")
    ap.add_argument("--cpu-only", action="store_true", help="the demonstration on the restatement alone")
    ap.add_argument("--noise", type=float, default=4.0)
    ap.add_argument("--max-steps", type=int, default=400)
    ap.add_argument("--cases", nargs="+", default=["1024x1", "2048x1", "4096x1", "4096x3"], help="side x channels")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    if args.demo:
        for image in ("disks", "nested"):
            rows.append(demo(image, args.noise, args.max_steps, not args.cpu_only))
            print(json.dumps(rows[-1]), flush=True)
    if args.cost:
        for case in args.cases:
            n, ch = (int(x) for x in case.split("x"))
            rows.append(cost(n, ch, args.reps, args.warmup))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
