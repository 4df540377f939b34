#!/usr/bin/env python3
"""What does measuring the mask's components cost on the GPU, beside labelling them and beside the old way?  Records, asserts nothing.
For n x n contexts (1024, 2048, 4096 with one channel, 4096 with three) and two level sets --
  noisy    a noisy disk after 50 iterations from the checkerboard: many components;
  inside   the plane set wholly inside: ONE component, every run adds to the same row -- the worst contention --
  measure_us      the HOST clock around `reps` cvh_measure calls with a full table (cap = K) after `warmup` calls; every call ends in its
                  two host waits, which are inside the number
  components_us   the same around cvh_components with a full table (one add and up to four min / max per run: the yardstick for the atomics)
  cpu_*_ms        the old way, once: cvh_get_mask and cvh_get_image (across PCIe), then the numpy restatement (tests/measure_util.py)
The rows of the two ways are compared (`agree`).  Prints one JSON line per case and writes them to --out.

    python tools/measure_probe.py [--sizes 1024 2048 4096] [--reps 20] [--warmup 3] [--no-cpu] [--out measure_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from chan_vese_amd import capi, synth  # noqa: E402
import measure_util as mu  # noqa: E402


def per_call(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def probe(n, channels, kind, reps, warmup, cpu):
    with capi.Context(n, n, channels, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([synth.disk(n, 200 - 30 * k, 50 + 20 * k, noise=48, seed=7 + k) for k in range(channels)])
        if kind == "noisy":
            ctx.init_checkerboard()
            ctx.run(50)
        else:
            ctx.set_levelset(np.ones((n, n)))
        k, table = ctx.measure()
        row = {"probe": "measure", "n": n, "channels": channels, "levelset": kind, "K": k, "clock": "host, around the call and its waits",
               "reps": reps, "warmup": warmup,
               "measure_us": round(per_call(lambda: ctx.measure(cap=max(k, 1)), reps, warmup) * 1e6, 1),
               "components_us": round(per_call(lambda: ctx.components(cap=max(k, 1)), reps, warmup) * 1e6, 1),
               "count_only_us": round(per_call(lambda: ctx.measure(cap=0), reps, warmup) * 1e6, 1)}
        if cpu:
            t0 = time.perf_counter()
            mask = ctx.get_mask() != 0
            planes = ctx.get_image()
            t1 = time.perf_counter()
            want = mu.measure(mask, planes, 4)
            t2 = time.perf_counter()
            row.update(cpu_fetch_ms=round((t1 - t0) * 1e3, 1), cpu_numpy_ms=round((t2 - t1) * 1e3, 1), cpu_total_ms=round((t2 - t0) * 1e3, 1),
                       agree=bool(want.tobytes() == table.tobytes()))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[1024, 2048, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    capi.lib()
    rows = []
    cases = [(n, 1) for n in args.sizes] + ([(4096, 3)] if 4096 in args.sizes else [])
    for n, channels in cases:
        for kind in ("noisy", "inside"):
            rows.append(probe(n, channels, kind, args.reps, args.warmup, not args.no_cpu))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
