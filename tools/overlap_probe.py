#!/usr/bin/env python3
"""What does the contingency table of the mask's components against a second label plane cost on the GPU, and what did the same rows
cost the old way?  Records, asserts nothing.
For n x n one-channel contexts (1024, 2048, 4096), two level sets -- a noisy disk after 50 iterations from the checkerboard, and the plane
wholly inside (one component: every run adds to few pairs, the contended case) -- against two truth planes already in device memory: the
clean disk's labels, and a grid of 32 x 32-pixel squares with distinct labels.
  overlaps_us       the HOST clock around `reps` cvh_overlaps_device calls with a full table after `warmup` calls (the context's pair table
                    has grown to its content by then); every call ends in its host waits and the host's sort, which are inside the number
  count_only_us     the same without a table (cap = 0): one wait, no rows, no sort
  old_*_ms          the round trip the call replaces, on the interface before it, `cpu_reps` times (the best is kept): cvh_components with
                    a device label plane, the plane fetched (4 bytes per pixel across PCIe), np.unique over the h w pairs as 64-bit keys
The rows of the two ways are compared (`agree`).  Prints one JSON line per case and writes them to --out.

    python tools/overlap_probe.py [--sizes 1024 2048 4096] [--reps 20] [--warmup 3] [--cpu-reps 2] [--out overlap_probe.json]
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

from chan_vese_amd import capi, synth  # noqa: E402


def hip_runtime():
    """the HIP runtime the library already loaded (no second one enters the process)"""
    capi.lib()
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    L = C.CDLL(path, mode=os.RTLD_NOLOAD | os.RTLD_NOW)
    L.hipMalloc.argtypes, L.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return L


def per_call(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def old_way(hip, ctx, d_labels, truth):
    t = {}
    n = ctx.h * ctx.w
    t0 = time.perf_counter()
    k, _ = ctx.components(4, False, labels_ptr=d_labels, cap=0)
    t["components"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    lab = np.empty(n, np.int32)
    assert hip.hipMemcpy(lab.ctypes.data, d_labels, 4 * n, 2) == 0
    t["fetch"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    keys, counts = np.unique((lab.astype(np.int64) << 32) | truth.reshape(-1).view(np.uint32).astype(np.int64), return_counts=True)
    rows = np.zeros(keys.size, capi.OVERLAP_DTYPE)
    rows["a"], rows["b"], rows["count"] = keys >> 32, (keys & 0xffffffff).astype(np.uint32).view(np.int32), counts
    rows = rows[np.lexsort((rows["b"], rows["a"]))]
    t["unique"] = time.perf_counter() - t0
    return rows, k, t


def probe(hip, n, reps, warmup, cpu_reps):
    clean = synth.disk(n)
    yy, xx = np.mgrid[0:n, 0:n]
    truths = {"disk": np.ascontiguousarray((clean > 125).astype(np.int32)), "grid32": ((yy // 32) * ((n + 31) // 32) + xx // 32 + 1).astype(np.int32)}
    bufs = {}
    for name in list(truths) + ["labels"]:
        bufs[name] = C.c_void_p()
        assert hip.hipMalloc(C.byref(bufs[name]), 4 * n * n) == 0
    for name, t in truths.items():
        assert hip.hipMemcpy(bufs[name], t.ctypes.data, t.nbytes, 1) == 0
    out = []
    try:
        for levelset in ("noisy disk after 50 iterations", "wholly inside"):
            with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as ctx:
                ctx.set_image([synth.disk(n, noise=48, seed=7)])
                if levelset == "wholly inside":
                    ctx.set_levelset(np.ones((n, n)))
                else:
                    ctx.init_checkerboard()
                    ctx.run(50)
                for name, truth in truths.items():
                    d = bufs[name].value
                    rows, k = ctx.overlaps(d)
                    row = {"probe": "overlap", "n": n, "levelset": levelset, "truth": name, "K": k, "P": int(rows.size),
                           "clock": "host, around the call, its waits and its sort", "reps": reps, "warmup": warmup,
                           "overlaps_us": round(per_call(lambda: ctx.overlaps(d, cap=rows.size), reps, warmup) * 1e6, 1),
                           "count_only_us": round(per_call(lambda: ctx.overlaps(d, cap=0), reps, warmup) * 1e6, 1)}
                    best = None
                    for _ in range(cpu_reps):
                        t0 = time.perf_counter()
                        ref, k_ref, parts = old_way(hip, ctx, bufs["labels"].value, truth)
                        total = time.perf_counter() - t0
                        if best is None or total < best[0]:
                            best = (total, parts)
                    row["old_total_ms"] = round(best[0] * 1e3, 1)
                    row.update({f"old_{key}_ms": round(v * 1e3, 1) for key, v in best[1].items()})
                    row["cpu_reps"] = cpu_reps
                    row["agree"] = bool(k == k_ref and rows.tobytes() == ref.tobytes())
                    out.append(row)
                    print(json.dumps(row), flush=True)
    finally:
        for b in bufs.values():
            hip.hipFree(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[1024, 2048, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-reps", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    hip = hip_runtime()
    rows = []
    for n in args.sizes:
        rows += probe(hip, n, args.reps, args.warmup, args.cpu_reps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
