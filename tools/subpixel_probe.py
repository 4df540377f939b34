#!/usr/bin/env python3
"""What does the subpixel polygon of the zero level cost on the GPU, beside the lattice loops of the same level set and beside the old way?
Records, asserts nothing.
For n x n one-channel contexts (1024, 2048, 4096) and two level sets --
  noisy    a noisy disk after 50 iterations from the checkerboard: many loops;
  inside   the plane set wholly inside: ONE loop, every edge a plane-border edge (the midpoint, no division) --
  subpixel_us     the HOST clock around `reps` cvh_contours_subpixel_device calls with full outputs (loop table on the host, points in
                  device memory, caps = the counts) after `warmup` calls; every call ends in its two host waits, inside the number
  lattice_us      the same around cvh_contours_device(simplify = 0) on the same level set, in the same process: the same launches but the
                  last, 8 bytes per point and not 16
  cpu_*_ms        the round trip the call replaces, once: cvh_get_levelset (8 bytes per pixel across PCIe), then the restatement of
                  tests/subpixel_util.py -- its tracer is PLAIN PYTHON, the only CPU tracer this tree has; skipped above --cpu-edges edges or
                  --cpu-pixels pixels (it visits every foreground pixel)
The two ways are compared (`agree`).  Prints one JSON line per case and writes them to --out.

    python tools/subpixel_probe.py [--sizes 1024 2048 4096] [--reps 20] [--warmup 3] [--cpu-edges 1000000] [--cpu-pixels 1048576] [--out subpixel_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from chan_vese_amd import capi, synth  # noqa: E402
import subpixel_util as su  # noqa: E402
from contour_probe import device_buffer, per_call  # noqa: E402


def probe(n, kind, reps, warmup, cpu_edges, cpu_pixels):
    with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([synth.disk(n, 200, 50, noise=48, seed=7)])
        if kind == "noisy":
            ctx.init_checkerboard()
            ctx.run(50)
        else:
            ctx.set_levelset(np.ones((n, n)))
        loops, points = ctx.contours_subpixel()
        L, P = loops.size, points.shape[0]
        hip, d = device_buffer(16 * max(P, 1))
        table = np.zeros(max(L, 1), capi.CONTOUR_LOOP_DTYPE)
        nl, npts = C.c_long(0), C.c_long(0)
        lib = capi.lib()

        def subpixel():
            assert lib.cvh_contours_subpixel_device(ctx._h, 8, 0, 0, 0, 0, table.ctypes.data, L, d, P, C.byref(nl), C.byref(npts), None) == 0

        def lattice():
            assert lib.cvh_contours_device(ctx._h, 8, 0, 0, 0, 0, 0, table.ctypes.data, L, d, P, C.byref(nl), C.byref(npts), None) == 0

        row = {"probe": "subpixel", "n": n, "levelset": kind, "loops": L, "edges": P, "clock": "host, around the call and its waits",
               "reps": reps, "warmup": warmup,
               "subpixel_us": round(per_call(subpixel, reps, warmup) * 1e6, 1),
               "lattice_us": round(per_call(lattice, reps, warmup) * 1e6, 1),
               "subpixel_again_us": round(per_call(subpixel, reps, warmup) * 1e6, 1)}
        t0 = time.perf_counter()
        u = ctx.get_levelset()
        t1 = time.perf_counter()
        row["cpu_fetch_ms"] = round((t1 - t0) * 1e3, 1)
        if P <= cpu_edges and n * n <= cpu_pixels:
            want = su.trace_subpixel(u, 8)
            t2 = time.perf_counter()
            row.update(cpu_trace_ms=round((t2 - t1) * 1e3, 1), cpu_total_ms=round((t2 - t0) * 1e3, 1), cpu_tracer="plain Python",
                       agree=bool(want[0].tobytes() == loops.tobytes() and want[1].tobytes() == points.tobytes()))
        else:
            row.update(cpu_trace_ms=None, cpu_total_ms=None, cpu_tracer="plain Python", agree=None)
        hip.hipFree(d)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[1024, 2048, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-edges", type=int, default=1000000)
    ap.add_argument("--cpu-pixels", type=int, default=1 << 20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    capi.lib()
    rows = []
    for n in args.sizes:
        for kind in ("noisy", "inside"):
            rows.append(probe(n, kind, args.reps, args.warmup, args.cpu_edges, args.cpu_pixels))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
