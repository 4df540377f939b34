#!/usr/bin/env python3
"""What does tracing the mask's boundary into ordered loops cost on the GPU, beside labelling its components, beside one iteration and
beside the old way?  Records, asserts nothing.
For n x n one-channel contexts (1024, 2048, 4096) and two level sets --
  noisy    a noisy disk after 50 iterations from the checkerboard: many loops;
  inside   the plane set wholly inside: ONE loop, every edge adds to the same row -- the contended case --
  contours_us     the HOST clock around `reps` cvh_contours_device calls with full outputs (loop table on the host, points in device
                  memory, caps = the counts) after `warmup` calls; every call ends in its two host waits, which are inside the number
  counts_us       the same with no outputs (no scatter launch, no rows)
  host_form_us    the same around cvh_contours (points to host memory)
  all_vertices_us contours_us with simplify = 0
  components_us   the same around cvh_components with a full table
  csv_iteration_us   one iteration of the same plane: the host clock around 100 enqueued iterations and their wait, over 100
  cpu_*_ms        the old way, once: cvh_get_mask (across PCIe), then the sequential tracer of tests/contour_util.py (plain Python: the
                  only CPU tracer this tree has; skipped above --cpu-edges edges)
The two ways are compared (`agree`).  Prints one JSON line per case and writes them to --out.

    python tools/contour_probe.py [--sizes 1024 2048 4096] [--reps 20] [--warmup 3] [--cpu-edges 400000] [--out contour_probe.json]
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
import contour_util as ct  # noqa: E402


def per_call(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def device_buffer(nbytes):
    hip = None
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                hip = C.CDLL(line.split()[-1])
                break
    p = C.c_void_p()
    assert hip is not None and hip.hipMalloc(C.byref(p), max(int(nbytes), 8)) == 0
    return hip, p


def probe(n, kind, reps, warmup, cpu_edges):
    with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([synth.disk(n, 200, 50, noise=48, seed=7)])
        if kind == "noisy":
            ctx.init_checkerboard()
            ctx.run(50)
        else:
            ctx.set_levelset(np.ones((n, n)))
        loops, points = ctx.contours()
        L, P = loops.size, points.shape[0]
        P0 = ctx.contour_counts(simplify=False)[1]
        hip, d = device_buffer(8 * max(P0, 1))
        table = np.zeros(max(L, 1), capi.CONTOUR_LOOP_DTYPE)
        pts = np.zeros((max(P0, 1), 2), np.int32)
        nl, npts = C.c_long(0), C.c_long(0)
        lib = capi.lib()

        def device(simplify, outputs=True):
            rc = lib.cvh_contours_device(ctx._h, 8, 0, 0, 0, 0, simplify, table.ctypes.data if outputs else None, L, d if outputs else None,
                                         P if simplify else P0, C.byref(nl), C.byref(npts), None)
            assert rc == 0

        def host():
            assert lib.cvh_contours(ctx._h, 8, 0, 0, 0, 0, 1, table.ctypes.data, L, pts.ctypes.data, P, C.byref(nl), C.byref(npts)) == 0

        k, _ = ctx.components()
        row = {"probe": "contours", "n": n, "levelset": kind, "loops": L, "edges": int(loops["edges"].sum()), "points": P, "components": k,
               "clock": "host, around the call and its waits", "reps": reps, "warmup": warmup,
               "contours_us": round(per_call(lambda: device(1), reps, warmup) * 1e6, 1),
               "counts_us": round(per_call(lambda: device(1, False), reps, warmup) * 1e6, 1),
               "host_form_us": round(per_call(host, reps, warmup) * 1e6, 1),
               "all_vertices_us": round(per_call(lambda: device(0), reps, warmup) * 1e6, 1),
               "components_us": round(per_call(lambda: ctx.components(cap=max(k, 1)), reps, warmup) * 1e6, 1)}
        if row["edges"] <= cpu_edges:
            t0 = time.perf_counter()
            mask = ctx.get_mask() != 0
            t1 = time.perf_counter()
            want = ct.trace(mask, 8, True)
            t2 = time.perf_counter()
            row.update(cpu_fetch_ms=round((t1 - t0) * 1e3, 1), cpu_trace_ms=round((t2 - t1) * 1e3, 1), cpu_total_ms=round((t2 - t0) * 1e3, 1),
                       agree=bool(want[0].tobytes() == loops.tobytes() and np.array_equal(want[1], points)))
        else:
            t0 = time.perf_counter()
            ctx.get_mask()
            row.update(cpu_fetch_ms=round((time.perf_counter() - t0) * 1e3, 1), cpu_trace_ms=None, cpu_total_ms=None, agree=None)

        def iterate():
            ctx.enqueue_steps(100)
            ctx.sync()
        row["csv_iteration_us"] = round(per_call(iterate, 3, 1) * 1e4, 1)
        hip.hipFree(d)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[1024, 2048, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-edges", type=int, default=400000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    capi.lib()
    rows = []
    for n in args.sizes:
        for kind in ("noisy", "inside"):
            rows.append(probe(n, kind, args.reps, args.warmup, args.cpu_edges))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
