#!/usr/bin/env python3
"""Device-memory I/O against the host-buffer calls, whole pipeline and parts, in ONE process, A and B alternating.

  (A) the pipeline as INTEGRATION.md 5 times it: per-member set_image from numpy, perona_malik_batch, per-member init_checkerboard,
      run_batch, per-member get_mask to numpy;
  (B) the same through set_image_device_batch / init_checkerboard_batch / get_mask_device_batch on device-resident sources and sinks
      (torch tensors; B's egress time ends with a synchronise of the caller's stream, so the masks exist when the clock stops).

Wall time (host clock; every part ends in a device synchronise) of the parts and the whole, min / median / max over the repetitions.
Bar at 64 x 256^2 (README example 1: -S -L 0.25 -T 100 -K 30 -N 70): B's non-compute part (everything outside the Perona-Malik and CSV
batch calls) below A's by more than A's own max - min spread, and B's compute parts within that spread of A's.  Exit status 1 if it fails.

Measured on one MI355X (profiles/r08_device_io/device_io_probe.txt; median ms, A -> B): outside the compute calls 64 x 256^2 7.50 -> 1.92
(A's spread 1.42; compute 14.73 / 14.36), 16 x 480 x 640 x 3 6.81 -> 2.34, 8 x 1024^2 2.09 -> 0.47, 1 x 4096^2 0.98 -> 0.29 of a 16 ms
pipeline -- no gain worth the name there.  Three-channel stop-norm fetch at 16 x 480 x 640 x 3: 0.93 ms of the 1.42 ms ingest.

usage: python tools/device_io_probe.py [--reps 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch  # noqa: E402  (before chan_vese_amd: one HIP runtime)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chan_vese_amd import capi, synth  # noqa: E402

PM = (30.0, 0.25, 100.0)
STEPS = 70
PARTS = ["ingest", "perona_malik", "init", "run", "egress"]


def images(n, h, w, c):
    return [np.stack([synth.disk(h, 200 - (3 * i) % 60 - 20 * k, 40 + (5 * i) % 40 + 10 * k, noise=8, seed=7 * i + k, h=h, w=w) for k in range(c)])
            for i in range(n)]


def clock(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def run_a(ctxs, imgs):
    t = {}
    t["ingest"] = clock(lambda: [c.set_image(list(im)) for c, im in zip(ctxs, imgs)])
    t["perona_malik"] = clock(lambda: capi.perona_malik_batch(ctxs, *PM))
    t["init"] = clock(lambda: [c.init_checkerboard() for c in ctxs])
    t["run"] = clock(lambda: capi.run_batch(ctxs, STEPS))
    masks = []
    t["egress"] = clock(lambda: masks.extend(c.get_mask() for c in ctxs))
    return t, masks


def run_b(ctxs, src, sink):
    stream = torch.cuda.current_stream().cuda_stream
    t = {}
    t["ingest"] = clock(lambda: capi.set_image_device_batch(ctxs, [s.data_ptr() for s in src], capi.LAYOUT_PLANAR, stream))
    t["perona_malik"] = clock(lambda: capi.perona_malik_batch(ctxs, *PM))
    t["init"] = clock(lambda: capi.init_checkerboard_batch(ctxs))
    t["run"] = clock(lambda: capi.run_batch(ctxs, STEPS))

    def egress():
        capi.get_mask_device_batch(ctxs, [s.data_ptr() for s in sink], False, stream)
        torch.cuda.current_stream().synchronize()
    t["egress"] = clock(egress)
    return t


def stats(v):
    return min(v), statistics.median(v), max(v)


def measure(n, h, w, c, reps, say):
    imgs = images(n, h, w, c)
    a_ctx = [capi.Context(h, w, c) for _ in range(n)]
    b_ctx = [capi.Context(h, w, c) for _ in range(n)]
    src = [torch.from_numpy(im).cuda() for im in imgs]
    sink = [torch.empty((h, w), dtype=torch.uint8, device="cuda") for _ in range(n)]
    ta = {k: [] for k in PARTS + ["whole", "non_compute", "compute"]}
    tb = {k: [] for k in PARTS + ["whole", "non_compute", "compute"]}
    for rep in range(reps + 1):             # repetition 0 warms both (code objects, tables, pinned staging) and checks B against A
        a, masks = run_a(a_ctx, imgs)
        b = run_b(b_ctx, src, sink)
        if rep == 0:
            for m, s in zip(masks, sink):
                assert np.array_equal(m, s.cpu().numpy()), "B's masks differ from A's"
            continue
        for t, acc in ((a, ta), (b, tb)):
            for k in PARTS:
                acc[k].append(t[k])
            acc["whole"].append(sum(t.values()))
            acc["compute"].append(t["perona_malik"] + t["run"])
            acc["non_compute"].append(t["ingest"] + t["init"] + t["egress"])
    say(f"## {n} x {h} x {w} x {c}   (Perona-Malik K={PM[0]:g} L={PM[1]:g} T={PM[2]:g}, {STEPS} iterations, {reps} repetitions, ms: min / median / max)")
    for k in PARTS + ["non_compute", "compute", "whole"]:
        sa, sb = stats(ta[k]), stats(tb[k])
        say(f"  {k:13s} A {sa[0]:9.3f} {sa[1]:9.3f} {sa[2]:9.3f}   B {sb[0]:9.3f} {sb[1]:9.3f} {sb[2]:9.3f}   A/B median {sa[1] / sb[1]:6.2f}x")
    if c == 3:
        # the three-channel stop-norm fetch: the same bytes as 3n one-channel members stay on the device (exact integer sums)
        one = [capi.Context(h, w, 1) for _ in range(3 * n)]
        flat = [s[k] for s in src for k in range(3)]
        stream = torch.cuda.current_stream().cuda_stream
        t1, t3 = [], []
        for rep in range(reps + 1):
            x1 = clock(lambda: capi.set_image_device_batch(one, [s.data_ptr() for s in flat], capi.LAYOUT_PLANAR, stream))
            x3 = clock(lambda: capi.set_image_device_batch(b_ctx, [s.data_ptr() for s in src], capi.LAYOUT_PLANAR, stream))
            if rep:
                t1.append(x1)
                t3.append(x3)
        s1, s3 = stats(t1), stats(t3)
        say(f"  three-channel stop-norm fetch: ingest of {n} three-channel members {s3[0]:.3f} / {s3[1]:.3f} / {s3[2]:.3f} ms, of the same planes as "
            f"{3 * n} one-channel members {s1[0]:.3f} / {s1[1]:.3f} / {s1[2]:.3f} ms: the fetch and the host's serial sums cost {s3[1] - s1[1]:.3f} ms (median)")
        for x in one:
            x.close()
    if n > 1:
        # N calls of the single-context set_levelset_device (no batched form): what they cost beside the checkerboard batch
        u = torch.zeros((h, w), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        ts = [clock(lambda: [x.set_levelset_device(u.data_ptr(), 64, stream) for x in b_ctx]) for _ in range(reps + 1)][1:]
        s = stats(ts)
        say(f"  {n} calls of set_levelset_device: {s[0]:.3f} / {s[1]:.3f} / {s[2]:.3f} ms (init_checkerboard_batch: {stats(tb['init'])[1]:.3f})")
    for x in a_ctx + b_ctx:
        x.close()
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-first", action="store_true", help="64 x 256^2 only")
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("at least five repetitions")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# device_io_probe: {capi.lib().cvh_version().decode()}, {torch.cuda.get_device_name(0)}")
    ok = True
    sizes = [(64, 256, 256, 1), (16, 480, 640, 3), (8, 1024, 1024, 1), (1, 4096, 4096, 1)]
    for i, (n, h, w, c) in enumerate(sizes[:1] if args.only_first else sizes):
        ta, tb = measure(n, h, w, c, args.reps, say)
        if i == 0:
            spread_nc = max(ta["non_compute"]) - min(ta["non_compute"])
            gain = statistics.median(ta["non_compute"]) - statistics.median(tb["non_compute"])
            spread_c = max(ta["compute"]) - min(ta["compute"])
            diff_c = abs(statistics.median(ta["compute"]) - statistics.median(tb["compute"]))
            p1, p2 = gain > spread_nc, diff_c <= spread_c
            say(f"  BAR non-compute: A - B = {gain:.3f} ms against A's spread {spread_nc:.3f} ms: {'PASS' if p1 else 'FAIL'}")
            say(f"  BAR compute: |A - B| = {diff_c:.3f} ms against A's spread {spread_c:.3f} ms: {'PASS' if p2 else 'FAIL'}")
            ok = p1 and p2
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
