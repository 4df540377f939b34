#!/usr/bin/env python3
"""What does the Gaussian blur cost on the GPU, and what does a blurred edge map do for the geodesic run?  Records, asserts nothing.
Cost (the default): for n x n one-channel sources (n = 1024, 2048, 4096), us per cvh_smooth_planes call, BLUR 1 -> 1, at sigma = 1, 3,
10 and 21 (R = 3, 9, 30, 63) -- the HOST clock around `reps` calls after `warmup` calls; every call ends in its one host wait.  Beside
them, per size and in the same process: cvh_local_planes MEAN at the same R; the us of one CSV iteration of the same plane
(cvh_last_run_ms of a 64-iteration enqueue, the second of two); and the round trip the call replaces -- cvh_get_image,
scipy.ndimage.gaussian_filter(mode="nearest", truncate=3) on the host, cvh_set_image --, ONE round each.  Device times of the kernels
alone are not taken.
Demonstration (--demo): the geodesic scene of the README (tests/geodesic_util.py: 64 x 64, a square with a 3 px arm, noise sigma 20),
mu = 5 and 20, K of DEMO_KS, with the edge map built from G_sigma * I for sigma = 1 and 2 (smooth_util's restatement of the blur), beside
the recorded map of the Perona-Malik-smoothed plane: IoU with the clean shape, speckle count, share of the arm kept -- on the CPU
restatement, and with the same runs on the card (--cpu-only: the restatement alone) whether the card's mask is the restatement's.
Prints one JSON line per row and writes them to --out.

    python tools/smooth_probe.py [--demo] [--cpu-only] [--sizes 1024 2048 4096] [--reps 20] [--warmup 3] [--out smooth_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIGMAS = (1.0, 3.0, 10.0, 21.0)
DEMO_SIGMAS, DEMO_MUS = (1.0, 2.0), (5.0, 20.0)


def per_call_us(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def cost(n, reps, warmup):
    from scipy import ndimage
    from chan_vese_amd import capi, synth
    plane = synth.disk(n, 180, 40, noise=16, seed=7)
    with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as src, capi.Context(n, n, 1) as dst:
        dst.set_option("co_resident", 0)
        src.set_image([plane])
        src.init_checkerboard()
        for _ in range(2):
            src.enqueue_steps(64)
            src.sync()
        row = {"probe": "smooth", "n": n, "clock": "host, around the call and its wait", "reps": reps, "warmup": warmup,
               "csv_iteration_us": round(src.last_run_ms() * 1000 / 64, 2), "blur_us": {}, "local_mean_same_radius_us": {}, "round_trip_us": {}}
        for sigma in SIGMAS:
            R = capi.gauss_taps(sigma)[0]
            key = f"sigma={sigma:g} R={R}"
            row["blur_us"][key] = round(per_call_us(lambda: src.smooth_planes_to(dst, sigma, "blur"), reps, warmup), 1)
            row["local_mean_same_radius_us"][key] = round(per_call_us(lambda: src.local_planes_to(dst, R, "mean"), reps, warmup), 1)
            row["round_trip_us"][key] = round(per_call_us(
                lambda: dst.set_image([ndimage.gaussian_filter(src.get_image()[0], sigma, mode="nearest", truncate=3.0)]), 1, 0), 1)
            print("#", n, key, row["blur_us"][key], row["local_mean_same_radius_us"][key], row["round_trip_us"][key], flush=True)
    return row


def demo(on_card):
    import geodesic_util as G
    import smooth_util as U
    img, shape, arm = G.demo_scene()
    u0, t = G.demo_start(img)
    sources = {"perona-malik": G.demo_smoothed(img)}
    for sigma in DEMO_SIGMAS:
        sources[f"gauss sigma={sigma:g}"] = U.blur(img, U.gauss_taps(sigma)[1])
    rows = []
    for mu in DEMO_MUS:
        p = G.demo_params(mu)
        for K in G.DEMO_KS:
            for name, smooth in sources.items():
                gq = G.edge_map([smooth], K)
                m = G.mask(G.run([img], u0, gq, p, G.demo_steps(mu))[0])
                iou, speckle, kept = G.demo_score(m, shape, arm)
                row = {"probe": "smooth-demo", "map_from": name, "mu": mu, "K": K, "otsu": t, "steps": G.demo_steps(mu), "dt": G.demo_dt(mu),
                       "iou": round(iou, 4), "speckle": speckle, "arm_kept": round(kept, 3)}
                if on_card:
                    from chan_vese_amd import capi
                    params = capi.make_params(**{k: (list(v) if isinstance(v, tuple) else v) for k, v in p.items()})
                    with capi.Context(64, 64, 1, params) as c, capi.Context(64, 64, 1) as s:
                        c.set_image([img])
                        c.set_levelset(u0)
                        if name.startswith("gauss"):
                            c.smooth_planes_to(s, float(name.split("=")[1]), "blur")
                        else:
                            s.set_image([img])
                            s.perona_malik(*G.DEMO_PM)
                        row["card_map_source_equals_cpu"] = bool(np.array_equal(s.get_image()[0], smooth))
                        c.edge_map_from(s, K)
                        capi.geodesic_run(c, G.demo_steps(mu))
                        got = c.get_mask()
                    ci, cs, ck = G.demo_score(got != 0, shape, arm)
                    row.update(card_iou=round(ci, 4), card_speckle=cs, card_arm_kept=round(ck, 3), card_mask_differs_at=int(((got != 0) != m.astype(bool)).sum()))
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--demo", action="store_true")
    ap.add_argument("--cpu-only", action="store_true", help="the demonstration on the restatement alone")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048, 4096])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    rows = []
    if args.demo:
        rows += demo(not args.cpu_only)
    else:
        for n in args.sizes:
            rows.append(cost(n, args.reps, args.warmup))
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
