#!/usr/bin/env python3
"""What does a colour conversion cost on the GPU?  Records, asserts nothing.
For n x n three-channel contexts (n = 1024, 2048, 4096): us per cvh_convert_colour call and per cvh_luma_image call -- the HOST clock
around `reps` calls after `warmup` calls; every call ends in its one host wait, and a convert call, like every call that replaces the
planes of a three-channel context, also fetches the planes and takes the stop norm on the host behind that wait, which is inside the
number -- beside the us of one CSV iteration of the same three-channel plane in the same process (cvh_last_run_ms of a 64-iteration
enqueue, the second of two) and beside the time 6 (convert) and 4 (luma) bytes per pixel take at the README's measured copy rate
(285 MB in 42 - 48 us: 6.3 TB/s).  Prints one JSON line per size and writes them to --out.

    python tools/colour_probe.py [--sizes 1024 2048 4096] [--reps 20] [--warmup 3] [--out colour_probe.json]
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


def probe(n, reps, warmup):
    planes = [synth.disk(n, 180 - 60 * k, 40 + 80 * k, noise=16, seed=7 + k) for k in range(3)]
    with capi.Context(n, n, 3, capi.make_params(tol=0.0)) as ctx, capi.Context(n, n, 1) as grey:
        grey.set_option("co_resident", 0)
        ctx.set_image(planes)
        ctx.init_checkerboard()
        for _ in range(2):
            ctx.enqueue_steps(64)
            ctx.sync()
        row = {"probe": "colour", "n": n, "channels": 3, "clock": "host, around the call and its wait", "reps": reps, "warmup": warmup,
               "csv_iteration_us": round(ctx.last_run_ms() * 1000 / 64, 2),
               "luma_us": round(per_call_us(lambda: ctx.luma_to(grey, "bgr"), reps, warmup), 1),
               "luma_4_bytes_per_pixel_at_copy_rate_us": round(4.0 * n * n / COPY_BYTES_PER_US, 2),
               # (planes are bytes: converting again and again is well defined, and every call moves the same 6 bytes per pixel)
               "convert_us": round(per_call_us(lambda: ctx.convert_colour("ycrcb", "bgr"), reps, warmup), 1),
               "convert_6_bytes_per_pixel_at_copy_rate_us": round(6.0 * n * n / COPY_BYTES_PER_US, 2)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for n in args.sizes:
        rows.append(probe(n, args.reps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
