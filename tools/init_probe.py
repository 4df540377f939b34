#!/usr/bin/env python3
"""What does an Otsu start buy?  For synthetic noisy disks (chan_vese_amd.synth.disk, radius n / 4, noise 32) at 256^2 and 512^2 with 1 and
3 channels: iterations until the stop rule fires (default parameters, tol 1e-3) and the IoU of the final mask with the synthetic disk,
from the checkerboard start and from the Otsu start (+1 above Otsu's threshold of the grey values, -1 elsewhere) -- on the CPU oracle,
and on the GPU when one is present.  The oracle's Otsu start is built here from the definition in include/chanvese_hip.h (numpy
histogram, the library's host helper cvh_otsu_from_histogram for the threshold); the GPU's is cvh_init_otsu, whose threshold is recorded
beside it.  Prints one JSON line per case and writes them to --out.  Records, asserts nothing.

    python tools/init_probe.py [--sizes 256 512] [--max-steps 2000] [--out init_probe.json] [--no-gpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chan_vese_amd import capi as C, synth  # noqa: E402


def iou(mask, truth):
    """of the mask or of its complement, whichever side the run called 'inside'"""
    m = mask.astype(bool)
    best = 0.0
    for cand in (m, ~m):
        union = (cand | truth).sum()
        best = max(best, float((cand & truth).sum()) / float(union) if union else 1.0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--max-steps", type=int, default=2000)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-gpu", action="store_true")
    args = ap.parse_args()
    from oracle import cv_oracle as O
    O.lib()
    capi = None
    if not args.no_gpu and C.device_count() > 0:
        capi = C
    rows = []
    for n in args.sizes:
        ii = np.arange(n)[:, None] - n // 2
        jj = np.arange(n)[None, :] - n // 2
        truth = ii * ii + jj * jj <= (n // 4) ** 2
        for channels in (1, 3):
            planes = [synth.disk(n, 200 - 30 * k, 50 + 20 * k, noise=32, seed=7 + k) for k in range(channels)]
            grey = np.sum([p.astype(np.int64) for p in planes], axis=0)
            t = C.otsu_from_histogram(np.bincount(grey.ravel(), minlength=255 * channels + 1))
            starts = {"checkerboard": O.checkerboard(n, n), "otsu": np.where(grey > t, 1.0, -1.0)}
            for start, u0 in starts.items():
                row = {"n": n, "channels": channels, "start": start, "otsu_t": t}
                t0 = time.perf_counter()
                u, done, _, _ = O.csv_run(planes, u0, O.make_params(), args.max_steps, trace=False)
                row["oracle"] = {"iterations": int(done), "stopped": bool(done < args.max_steps), "iou": round(iou(O.mask(u), truth), 6),
                                 "host_seconds": round(time.perf_counter() - t0, 3)}
                if capi is not None:
                    with capi.Context(n, n, channels) as ctx:
                        ctx.set_image(planes)
                        gpu_t = ctx.init_otsu() if start == "otsu" else None
                        if start != "otsu":
                            ctx.init_checkerboard()
                        done, _ = ctx.run(args.max_steps)
                        row["gpu"] = {"otsu_t": gpu_t, "iterations": int(done), "stopped": bool(ctx.sync()[2]), "iou": round(iou(ctx.get_mask(), truth), 6),
                                      "run_ms": round(ctx.last_run_ms(), 3)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
