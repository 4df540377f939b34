#!/usr/bin/env python3
"""What does the object split cost on the GPU, and what did the same labels cost the old way?  Records; asserts only that the two ways
give the same labels.
For n x n one-channel contexts (1024, 2048, 4096) and two scenes -- a noisy disk after 50 iterations from the checkerboard, and a field
of touching disks built for each radius (disk radius 2 R, necks about R wide: every case splits) -- split at R = 4, 16 and 64
(r2 = R^2), conn = 4:
  split_us          the HOST clock around `reps` cvh_split calls with full outputs (label plane and a table of K rows) after `warmup`
                    calls; the call's host waits are inside it
  sweeps            growth sweeps that ran in one such call (cvh_debug_split_sweeps)
  components_us     the same around cvh_components with a label plane and a full table, on the same level set
  erode_us          the same around cvh_get_mask_morph_device(ERODE, r2) followed by the wait for the stream
  trip_*_ms         the round trip the call replaces, for planes of at most --trip-max pixels a side (the numpy growth is rounds of
                    whole-plane minima: minutes at 4096^2): cvh_get_mask, the numpy restatement's erosion, labelling and growth
                    (tests/split_util.py), cvh_init_mask of the pieces
The labels of the two ways are compared wherever the round trip ran: a mismatch is an AssertionError.  Prints one JSON line per size
and writes them to --out.

    python tools/split_probe.py [--sizes 1024 2048 4096] [--radii 4 16 64] [--reps 20] [--warmup 3] [--trip-max 1024] [--out split_probe.json]
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


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--radii", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--trip-max", type=int, default=1024)
    ap.add_argument("--out", default="split_probe.json")
    a = ap.parse_args(argv)
    if min(a.sizes) < 64 or min(a.radii) < 0 or a.reps < 1 or a.warmup < 0 or a.iterations < 0:
        ap.error("sizes must be >= 64, radii >= 0, reps >= 1, warmup and iterations >= 0")
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


def per_call(fn, reps, warmup):
    total = 0.0
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if k >= warmup:
            total += time.perf_counter() - t0
    return total / reps


def touching_disks(n, radius):
    """a lattice of disks made for the split radius R: disk radius 2 R, neighbours overlapping by R / 8, so that the neck between two disks
    is about R wide (half-width sqrt(2 R * R / 8): the erosion by R cuts it) and every disk keeps a core of radius R"""
    r = 2 * max(radius, 1)
    pitch = 2 * r - max(1, radius // 8)
    y, x = np.mgrid[0:n, 0:n]
    cy, cx = (y % pitch) - pitch // 2, (x % pitch) - pitch // 2
    return cy * cy + cx * cx <= r * r


def probe(n, args, capi, synth, hip):
    import split_util as S
    sweeps = capi.lib().cvh_debug_split_sweeps
    sweeps.restype = C.c_ulong
    rec = {"n": n, "reps": args.reps, "warmup": args.warmup, "cases": []}
    labels, sink = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(labels), 4 * n * n) == 0 and hip.hipMalloc(C.byref(sink), n * n) == 0
    try:
        for scene in ("noisy_disk", "touching_disks"):
            with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as ctx:
                if scene == "noisy_disk":
                    ctx.set_image([synth.disk(n // 3, noise=48, seed=5, h=n, w=n)])
                    ctx.init_checkerboard()
                    ctx.enqueue_steps(args.iterations)
                    ctx.sync()
                for radius in args.radii:
                    r2 = radius * radius
                    if scene == "touching_disks":
                        ctx.set_levelset(np.where(touching_disks(n, radius), 1.0, -1.0))
                    if scene == "touching_disks" or radius == args.radii[0]:
                        k0, _ = ctx.components(labels_ptr=labels.value, cap=0)
                        comp_us = 1e6 * per_call(lambda: ctx.components(labels_ptr=labels.value, cap=k0), args.reps, args.warmup)
                    _, _, k = ctx.split(r2=r2, cap=0)
                    before = sweeps()
                    ctx.split(r2=r2, labels_ptr=labels.value, cap=k)
                    case = {"scene": scene, "R": radius, "K": k, "K_components": k0, "sweeps": int(sweeps() - before), "components_us": comp_us}
                    case["split_us"] = 1e6 * per_call(lambda: ctx.split(r2=r2, labels_ptr=labels.value, cap=k), args.reps, args.warmup)

                    def erode():
                        ctx.mask_morph("erode", r2=r2, out=sink.value)
                        assert hip.hipDeviceSynchronize() == 0
                    case["erode_us"] = 1e6 * per_call(erode, args.reps, args.warmup)
                    if n <= args.trip_max:
                        got = np.empty((n, n), np.int32)
                        assert hip.hipMemcpy(got.ctypes.data, labels, 4 * n * n, 2) == 0
                        t0 = time.perf_counter()
                        m = ctx.get_mask() != 0
                        t1 = time.perf_counter()
                        lab, kk, _ = S.split_numpy(m, 4, r2)
                        pieces = m & ~S.cut_of(lab)
                        t2 = time.perf_counter()
                        with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as other:
                            t2 = time.perf_counter()
                            other.init_mask(pieces.astype(np.uint8))
                            t3 = time.perf_counter()
                        case.update(trip_get_mask_ms=1e3 * (t1 - t0), trip_numpy_ms=1e3 * (t2 - t1), trip_init_mask_ms=1e3 * (t3 - t2),
                                    trip_total_ms=1e3 * (t3 - t0))
                        assert kk == k and np.array_equal(got, lab), (n, scene, radius, "device labels != restatement")
                        case["agree"] = True
                    print(f"{n} {scene} R={radius}: split {case['split_us']:.0f} us, {case['sweeps']} sweeps, K {k0} -> {k}, components "
                          f"{comp_us:.0f} us, erode {case['erode_us']:.0f} us" + (f", trip {case['trip_total_ms']:.0f} ms" if "trip_total_ms" in case else ""),
                          file=sys.stderr, flush=True)
                    rec["cases"].append(case)
    finally:
        hip.hipFree(labels)
        hip.hipFree(sink)
    return rec


def main(argv=None):
    args = parse_args(argv)
    from chan_vese_amd import capi, synth
    hip = hip_runtime(capi)
    hip.hipDeviceSynchronize.argtypes = []
    recs = []
    for n in args.sizes:
        rec = probe(n, args, capi, synth, hip)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in recs:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
