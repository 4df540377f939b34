#!/usr/bin/env python3
"""What do the local-statistics planes cost on the GPU?  Records, asserts nothing.
For n x n one-channel sources (n = 1024, 2048, 4096) and R = 2, 8, 32, 127: us per cvh_local_planes call for the 1 -> 1 deviation plane
and for the 1 -> 3 stack (copy, mean, deviation) -- the HOST clock around `reps` calls after `warmup` calls; every call ends in its one
host wait, and a stack call, like every call that replaces the planes of a three-channel context, also fetches the planes and takes the
stop norm on the host behind that wait, which is inside the number.  Beside them, per size: the us of one CSV iteration of the same plane
in the same process (cvh_last_run_ms of a 64-iteration enqueue, the second of two); the round trip the call replaces -- cvh_get_image, the
deviation plane from numpy cumulative sums on the host, cvh_set_image --, 3 rounds at R = 2; and the time the bytes the two passes move
take at the README's measured copy rate (285 MB in 42 - 48 us: 6.3 TB/s), without the band's start-up rows: 1 read + 6 written per pixel
in the row pass, 12 read + 1 written in the column pass (20 in all for the deviation plane); the stack reads the same sums once, reads the
plane for its copy and writes three (23).  Prints one JSON line per size and writes them to --out.

    python tools/local_probe.py [--sizes 1024 2048 4096] [--radii 2 8 32 127] [--reps 20] [--warmup 3] [--out local_probe.json]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chan_vese_amd import capi, synth  # noqa: E402

COPY_BYTES_PER_US = 285e6 / 45.0   # README: a plain copy of 285 MB takes 42 - 48 us
ISQRT = np.array([math.isqrt(q) for q in range(255 * 255 + 1)], dtype=np.uint8)


def per_call_us(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def host_deviation(plane, R):
    """the header's DEV from summed-area tables in int64"""
    h, w = plane.shape
    p = plane.astype(np.int64)
    r0, r1 = np.maximum(np.arange(h) - R, 0), np.minimum(np.arange(h) + R, h - 1) + 1
    c0, c1 = np.maximum(np.arange(w) - R, 0), np.minimum(np.arange(w) + R, w - 1) + 1

    def box(a):
        t = np.zeros((h + 1, w + 1), np.int64)
        t[1:, 1:] = a.cumsum(0).cumsum(1)
        return t[r1][:, c1] - t[r0][:, c1] - t[r1][:, c0] + t[r0][:, c0]

    n, S, Q = (r1 - r0)[:, None] * (c1 - c0)[None, :], box(p), box(p * p)
    return ISQRT[4 * (n * Q - S * S) // (n * n)]


def probe(n, radii, reps, warmup):
    plane = synth.disk(n, 180, 40, noise=16, seed=7)
    with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as src, capi.Context(n, n, 1) as one, capi.Context(n, n, 3) as three:
        for c in (one, three):
            c.set_option("co_resident", 0)
        src.set_image([plane])
        src.init_checkerboard()
        for _ in range(2):
            src.enqueue_steps(64)
            src.sync()

        def round_trip():
            one.set_image([host_deviation(src.get_image()[0], 2)])

        row = {"probe": "local", "n": n, "clock": "host, around the call and its wait", "reps": reps, "warmup": warmup,
               "csv_iteration_us": round(src.last_run_ms() * 1000 / 64, 2),
               "round_trip_get_numpy_set_R2_us": round(per_call_us(round_trip, 3, 1), 1),
               "dev_20_bytes_per_pixel_at_copy_rate_us": round(20.0 * n * n / COPY_BYTES_PER_US, 2),
               "stack_23_bytes_per_pixel_at_copy_rate_us": round(23.0 * n * n / COPY_BYTES_PER_US, 2),
               "dev_us": {}, "stack_us": {}}
        for R in radii:
            row["dev_us"][str(R)] = round(per_call_us(lambda: src.local_planes_to(one, R, "dev"), reps, warmup), 1)
            row["stack_us"][str(R)] = round(per_call_us(lambda: src.local_planes_to(three, R, "stack"), reps, warmup), 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--radii", type=int, nargs="+", default=[2, 8, 32, 127])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    for n in args.sizes:
        rows.append(probe(n, args.radii, args.reps, args.warmup))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
