#!/usr/bin/env python3
"""What does an energy call cost on the GPU?  Records, asserts nothing.
For n x n contexts (1024, 2048 and 4096 with one channel, 4096 with three): us per cvh_energy call -- the HOST clock around `reps` calls
after `warmup` calls; every call ends in its one host wait, which is inside the number -- with the means in the state block (behind a
run) and with the means taken inside the call (behind cvh_set_levelset: two launches more), beside the us of one CSV iteration of the
same plane in the same process (cvh_last_run_ms of a 64-iteration enqueue, the second of two) and beside the time 8 + C bytes per pixel
take at the README's measured copy rate (285 MB in 42 - 48 us: 6.3 TB/s).  Prints one JSON line per case and writes them to --out.

    python tools/energy_probe.py [--cases 1024x1 2048x1 4096x1 4096x3] [--reps 20] [--warmup 3] [--out energy_probe.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chan_vese_amd import capi, synth  # noqa: E402

COPY_BYTES_PER_US = 285e6 / 45.0   # README: a plain copy of 285 MB takes 42 - 48 us


def per_call_us(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def probe(n, channels, reps, warmup):
    planes = [synth.disk(n, 180 - 60 * k, 40 + 80 * k, noise=16, seed=7 + k) for k in range(channels)]
    with capi.Context(n, n, channels, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image(planes)
        ctx.init_checkerboard()
        for _ in range(2):
            ctx.enqueue_steps(64)
            ctx.sync()
        row = {"probe": "energy", "n": n, "channels": channels, "clock": "host, around the call and its wait", "reps": reps, "warmup": warmup,
               "csv_iteration_us": round(ctx.last_run_ms() * 1000 / 64, 2),
               "energy_us": round(per_call_us(ctx.energy, reps, warmup), 1),
               "bytes_per_pixel": 8 + channels,
               "bytes_at_copy_rate_us": round((8.0 + channels) * n * n / COPY_BYTES_PER_US, 2)}
        ctx.set_levelset(ctx.get_levelset())   # the means leave the state block: every call from here on takes them itself
        row["energy_with_means_us"] = round(per_call_us(ctx.energy, reps, warmup), 1)
        row["total"] = ctx.energy().total
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["1024x1", "2048x1", "4096x1", "4096x3"], help="side x channels")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for case in args.cases:
        n, channels = (int(v) for v in case.split("x"))
        rows.append(probe(n, channels, args.reps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
