#!/usr/bin/env python3
"""What do the rank planes cost on the GPU?  Records, asserts nothing.
For n x n one-channel sources (n = 1024, 2048, 4096): us per cvh_rank_planes call, 1 -> 1, for MEDIAN at R = 1, 2, 3, 7, MAX at
R = 2, 32, 127 and TOPHAT at R = 2, 32, 127, and for the 1 -> 3 triple (COPY, OPEN, TOPHAT) at R = 2, 32, 127 -- the HOST clock around
`reps` calls after `warmup` calls; every call ends in its one host wait, and the triple, like every call that replaces the planes of a
three-channel context, also fetches the planes and takes the stop norm on the host behind that wait, which is inside the number.  Beside
them, per size and from the same run: the us of one CSV iteration of the same plane (cvh_last_run_ms of a 64-iteration enqueue, the
second of two); the round trip each call replaces -- cvh_get_image, scipy.ndimage.median_filter / maximum_filter / white_tophat (grey
opening) with mode="nearest" on the host, cvh_set_image --, ONE round each; and the time the bytes the passes move take at the README's
measured copy rate (285 MB in 42 - 48 us: 6.3 TB/s): a row pass reads 1 and writes 1 byte per pixel, a column pass reads 3 and writes 2
(its hh goes through the workspace), the median reads 1 and writes 1, the writer of a median or a copy reads 1 and writes 1, a hat reads
the source once more -- MAX 7, TOPHAT 15, MEDIAN 4, the triple 18.  Device times of the kernels alone are not taken.  Prints one JSON
line per size and writes them to --out.

    python tools/rank_probe.py [--sizes 1024 2048 4096] [--reps 20] [--warmup 3] [--out rank_probe.json]
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

COPY_BYTES_PER_US = 285e6 / 45.0   # README: a plain copy of 285 MB takes 42 - 48 us
MEDIAN_RADII, FLAT_RADII = (1, 2, 3, 7), (2, 32, 127)
BYTES_PER_PIXEL = {"median": 4, "max": 7, "tophat": 15, "triple": 18}
TRIPLE = (capi.RANK_COPY, capi.RANK_OPEN, capi.RANK_TOPHAT)


def per_call_us(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def host_filter(plane, name, R):
    """the same bytes on the host: an extremum over mode="nearest" equals the truncated window; the median's borders differ (scipy pads,
    the header truncates), which changes no timing"""
    from scipy import ndimage
    size = 2 * R + 1
    if name == "median":
        return ndimage.median_filter(plane, size=size, mode="nearest")
    if name == "max":
        return ndimage.maximum_filter(plane, size=size, mode="nearest")
    return plane - ndimage.grey_opening(plane, size=(size, size), mode="nearest")


def probe(n, reps, warmup):
    plane = synth.disk(n, 180, 40, noise=16, seed=7)
    with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as src, capi.Context(n, n, 1) as one, capi.Context(n, n, 3) as three:
        for c in (one, three):
            c.set_option("co_resident", 0)
        src.set_image([plane])
        src.init_checkerboard()
        for _ in range(2):
            src.enqueue_steps(64)
            src.sync()
        row = {"probe": "rank", "n": n, "clock": "host, around the call and its wait", "reps": reps, "warmup": warmup,
               "csv_iteration_us": round(src.last_run_ms() * 1000 / 64, 2),
               "bytes_at_copy_rate_us": {k: round(v * n * n / COPY_BYTES_PER_US, 2) for k, v in BYTES_PER_PIXEL.items()},
               "median_us": {}, "max_us": {}, "tophat_us": {}, "triple_us": {}, "round_trip_us": {"median": {}, "max": {}, "tophat": {}}}
        for name, radii in (("median", MEDIAN_RADII), ("max", FLAT_RADII), ("tophat", FLAT_RADII)):
            for R in radii:
                row[name + "_us"][str(R)] = round(per_call_us(lambda: src.rank_planes_to(one, R, name), reps, warmup), 1)
                row["round_trip_us"][name][str(R)] = round(per_call_us(lambda: one.set_image([host_filter(src.get_image()[0], name, R)]), 1, 0), 1)
                print("#", n, name, R, row[name + "_us"][str(R)], row["round_trip_us"][name][str(R)], flush=True)
        for R in FLAT_RADII:
            row["triple_us"][str(R)] = round(per_call_us(lambda: src.rank_planes_to(three, R, TRIPLE), reps, warmup), 1)
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
