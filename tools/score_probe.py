#!/usr/bin/env python3
"""What does a mask score cost on the GPU, and what did the same score cost the old way?  Records, asserts nothing.
For n x n one-channel contexts (1024, 2048, 4096): a noisy disk after 50 iterations from the checkerboard, scored against the clean disk.
  score_device_us   the HOST clock around `reps` cvh_score_mask_device calls after `warmup` calls, the truth already in device memory;
                    every call ends in its one host wait, which is inside the number
  score_host_us     the same around cvh_score_mask: the truth's bytes cross PCIe inside the call
  cpu_*_ms          the old way, `cpu_reps` times: cvh_get_mask (one byte per pixel across PCIe), a numpy pass for the overlap counts, and
                    two scipy.ndimage.distance_transform_edt for the surface distances (binary_erosion for the surfaces)
The integers of the two ways are compared (`agree`); the CPU path's q16 sums are taken from the EDT's doubles, so `agree` covers the
counts, the maxima and the sums.  Prints one JSON line per size and writes them to --out.

    python tools/score_probe.py [--sizes 1024 2048 4096] [--reps 20] [--warmup 3] [--cpu-reps 2] [--out score_probe.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chan_vese_amd import capi, synth  # noqa: E402

CROSS = ndimage.generate_binary_structure(2, 1)


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


def cpu_score(ctx, truth, tol2):
    t = {}
    t0 = time.perf_counter()
    m = ctx.get_mask() != 0
    t["get_mask"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    tb = truth != 0
    out = dict(tp=int((m & tb).sum()), fp=int((m & ~tb).sum()), fn=int((~m & tb).sum()), tn=int((~m & ~tb).sum()))
    t["overlap"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    sm, st = m & ~ndimage.binary_erosion(m, CROSS, border_value=0), tb & ~ndimage.binary_erosion(tb, CROSS, border_value=0)
    t["surfaces"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    dm, dt = ndimage.distance_transform_edt(~st)[sm], ndimage.distance_transform_edt(~sm)[st]
    t["edt"] = time.perf_counter() - t0
    d2m, d2t = np.rint(dm * dm).astype(np.int64), np.rint(dt * dt).astype(np.int64)
    q = lambda d2: int(np.rint(np.sqrt(d2.astype(np.float64)) * 65536).astype(np.uint64).sum(dtype=np.uint64))
    out.update(surf_m=int(sm.sum()), surf_t=int(st.sum()), within_m=int((d2m <= tol2).sum()), within_t=int((d2t <= tol2).sum()),
               dist_m_q16=q(d2m), dist_t_q16=q(d2t), hd2_m=int(d2m.max()), hd2_t=int(d2t.max()), defined=1)
    return out, t


def probe(hip, n, reps, warmup, cpu_reps):
    clean = synth.disk(n)
    truth = np.ascontiguousarray((clean > 125).astype(np.uint8))
    d_truth = C.c_void_p()
    assert hip.hipMalloc(C.byref(d_truth), truth.size) == 0
    assert hip.hipMemcpy(d_truth, truth.ctypes.data, truth.size, 1) == 0
    try:
        with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as ctx:
            ctx.set_image([synth.disk(n, noise=48, seed=7)])
            ctx.init_checkerboard()
            ctx.run(50)
            s = ctx.score(d_truth.value)
            row = {"probe": "score", "n": n, "clock": "host, around the call and its wait", "reps": reps, "warmup": warmup,
                   "score_device_us": round(per_call(lambda: ctx.score(d_truth.value), reps, warmup) * 1e6, 1),
                   "score_host_us": round(per_call(lambda: ctx.score(truth), reps, warmup) * 1e6, 1)}
            best = None
            for _ in range(cpu_reps):
                t0 = time.perf_counter()
                ref, parts = cpu_score(ctx, truth, 4)
                total = time.perf_counter() - t0
                if best is None or total < best[0]:
                    best = (total, parts)
            row["cpu_total_ms"] = round(best[0] * 1e3, 1)
            row.update({f"cpu_{k}_ms": round(v * 1e3, 1) for k, v in best[1].items()})
            row["cpu_reps"] = cpu_reps
            got = {f: int(getattr(s, f)) for f in capi.SCORE_FIELDS}
            row["agree"] = got == ref
            row.update(iou=s.iou, dice=s.dice, hausdorff=s.hausdorff, assd=s.assd, surface_dice=s.surface_dice, surf_m=s.surf_m, surf_t=s.surf_t)
    finally:
        hip.hipFree(d_truth)
    return row


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
        rows.append(probe(hip, n, args.reps, args.warmup, args.cpu_reps))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
