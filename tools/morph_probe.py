#!/usr/bin/env python3
"""What does mask morphology cost on the GPU, and what did the same bytes cost the old way?  Records; asserts only that the two ways
give the same bytes.
For n x n one-channel contexts (1024, 2048, 4096): a noisy disk after 50 iterations from the checkerboard, opened and closed by the disk
dx^2 + dy^2 <= r2 for r2 = 2, 25 and 400.
  morph_device_us   the HOST clock around `reps` cvh_get_mask_morph_device calls after `warmup` calls, each followed by the wait for the
                    context's stream work (hipDeviceSynchronize): the call itself does not make the host wait, so the wait is added
  morph_levelset_us the same around cvh_morph_levelset (in place; its one host wait is inside the call); the level set is put back by
                    cvh_init_mask_device between calls, outside the clock
  init_mask_us      the same around cvh_init_mask_device (its one host wait inside), the bytes already in device memory
  cpu_*_ms          the path these replace, `cpu_reps` times: cvh_get_mask (one byte per pixel across PCIe), then
                    scipy.ndimage.binary_opening / binary_closing with the same disk -- binary_erosion(border_value=1) and
                    binary_dilation(border_value=0) in the order of the operation --, then cvh_set_levelset (eight bytes per pixel back)
The bytes of the two ways are compared for every (operation, r2): a mismatch is an AssertionError.  Prints one JSON line per size and
writes them to --out.

    python tools/morph_probe.py [--sizes 1024 2048 4096] [--r2 2 25 400] [--reps 20] [--warmup 3] [--cpu-reps 1] [--out morph_probe.json]
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

OPS = ("open", "close")


def disk_structure(r2):
    r = int(np.floor(np.sqrt(r2)))
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return y * y + x * x <= r2


def scipy_morph(mask, op, r2):
    """the header's open / close of a boolean plane in scipy's terms: erosion with border_value=1, dilation with border_value=0"""
    from scipy import ndimage
    d = disk_structure(r2)
    if op == "open":
        return ndimage.binary_dilation(ndimage.binary_erosion(mask, d, border_value=1), d, border_value=0)
    if op == "close":
        return ndimage.binary_erosion(ndimage.binary_dilation(mask, d, border_value=0), d, border_value=1)
    raise ValueError(f"op must be one of {OPS}, got {op!r}")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--r2", type=int, nargs="+", default=[2, 25, 400])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-reps", type=int, default=1)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--out", default="morph_probe.json")
    a = ap.parse_args(argv)
    if min(a.sizes) < 16 or min(a.r2) < 0 or max(a.r2) > 0xFFFFFFFF or a.reps < 1 or a.warmup < 0 or a.cpu_reps < 1 or a.iterations < 0:
        ap.error("sizes must be >= 16, r2 in 0 .. 2^32 - 1, reps and cpu-reps >= 1, warmup and iterations >= 0")
    return a


def hip_runtime(capi):
    """the HIP runtime the library already loaded (no second one enters the process)"""
    capi.lib()
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    L = C.CDLL(path, mode=os.RTLD_NOLOAD | os.RTLD_NOW)
    L.hipMalloc.argtypes, L.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return L


def per_call(fn, reps, warmup, between=None):
    """seconds per fn() over `reps` calls after `warmup`; between() runs outside the clock"""
    total = 0.0
    for k in range(warmup + reps):
        if between:
            between()
        t0 = time.perf_counter()
        fn()
        if k >= warmup:
            total += time.perf_counter() - t0
    return total / reps


def probe(n, args, capi, synth, hip):
    img = synth.disk(n // 3, noise=48, seed=5, h=n, w=n)
    rec = {"n": n, "iterations": args.iterations, "reps": args.reps, "warmup": args.warmup, "cpu_reps": args.cpu_reps, "cases": []}
    sink, start = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(sink), n * n) == 0 and hip.hipMalloc(C.byref(start), n * n) == 0
    try:
        with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as ctx:
            ctx.set_image([img])
            ctx.init_checkerboard()
            ctx.enqueue_steps(args.iterations)
            rec["steps"] = ctx.sync()[0]
            raw = ctx.get_mask()
            rec["foreground"] = int(raw.sum())
            assert hip.hipMemcpy(start, raw.ctypes.data, n * n, 1) == 0
            restore = lambda: ctx.init_mask(start.value, 1.0, -1.0)
            restore()                                                     # every case starts from the same +-1 level set
            rec["init_mask_us"] = 1e6 * per_call(restore, args.reps, args.warmup)
            out = np.empty((n, n), np.uint8)
            for op in OPS:
                for r2 in args.r2:
                    def device():
                        ctx.mask_morph(op, r2=r2, out=sink.value)
                        assert hip.hipDeviceSynchronize() == 0
                    case = {"op": op, "r2": r2, "morph_device_us": 1e6 * per_call(device, args.reps, args.warmup)}
                    assert hip.hipMemcpy(out.ctypes.data, sink, n * n, 2) == 0
                    case["morph_levelset_us"] = 1e6 * per_call(lambda: ctx.morph_levelset(op, r2=r2), args.reps, args.warmup, between=restore)
                    baked = ctx.get_mask()
                    restore()
                    t = {"get_mask": 0.0, "scipy": 0.0, "set_levelset": 0.0}
                    for _ in range(args.cpu_reps):
                        t0 = time.perf_counter()
                        m = ctx.get_mask() != 0
                        t1 = time.perf_counter()
                        cpu = scipy_morph(m, op, r2)
                        t2 = time.perf_counter()
                        ctx.set_levelset(np.where(cpu, 1.0, -1.0))
                        t3 = time.perf_counter()
                        t["get_mask"] += t1 - t0; t["scipy"] += t2 - t1; t["set_levelset"] += t3 - t2
                        restore()
                    for k, v in t.items():
                        case[f"cpu_{k}_ms"] = 1e3 * v / args.cpu_reps
                    case["cpu_total_ms"] = sum(case[f"cpu_{k}_ms"] for k in t)
                    case["foreground"] = int(out.sum())
                    assert np.array_equal(out, cpu.astype(np.uint8)), (n, op, r2, "device bytes != scipy bytes")
                    assert np.array_equal(baked, out), (n, op, r2, "level-set form != byte form")
                    case["agree"] = True
                    print(f"{n} {op} r2={r2}: device {case['morph_device_us']:.0f} us, cpu {case['cpu_total_ms']:.1f} ms", file=sys.stderr, flush=True)
                    rec["cases"].append(case)
    finally:
        hip.hipFree(sink)
        hip.hipFree(start)
    return rec


def main(argv=None):
    args = parse_args(argv)
    from chan_vese_amd import capi, synth
    hip = hip_runtime(capi)
    recs = []
    for n in args.sizes:
        rec = probe(n, args, capi, synth, hip)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    with open(args.out, "w") as f:
        json.dump(recs, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
