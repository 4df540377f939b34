#!/usr/bin/env python3
"""What does an iteration of the localised run (include/chanvese_hip.h, "Localised regions") cost on the GPU?  Records, asserts nothing.

Per plane (1024^2, 2048^2, 4096^2, 4096^2 x 3) and radius (2, 10, 32, 127): us per iteration -- cvh_last_run_ms of a 64-iteration
cvh_localized_run with tol = 0 and "sync_every" 64, the median of 20 timed calls after 3 -- beside an iteration of cvh_enqueue_steps of
the same plane in the same process in the per-launch flow ("resident" 0; 64-iteration enqueues, the same counts), their ratio, the
R = 127 to R = 2 ratio, and the bytes per pixel-iteration counted from the code (localized_kernels.hip):
    row pass   reads u (8) and the image (C), writes 1 + C horizontal sums (8 each)
    step       reads the entering and the leaving row of 1 + C sums (16 each), u (8), the image (C), T_k (4 C); writes u (8)
    = 48 + 30 C, whatever R (a strip's lead-in of 2 R + 1 rows, at most a third of its reads, and the row pass's 2 R span columns per
    1024 come on top).

Every plane runs in a child process of its own under a time limit; the first child that fails ends the probe.

    python tools/localized_probe.py [--cases 1024x1 2048x1 4096x1 4096x3] [--radii 2 10 32 127] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cost(n, channels, radii, reps, warmup):
    from chan_vese_amd import capi, synth
    planes = [synth.disk(n, 180 - 60 * k, 40 + 80 * k, noise=16, seed=7 + k) for k in range(channels)]
    rows = []
    with capi.Context(n, n, channels, capi.make_params(tol=0.0, mu=100.0)) as ctx:
        ctx.set_image(planes)
        ctx.set_option("sync_every", 64)
        ctx.set_option("resident", 0)
        ctx.init_checkerboard()
        single = []
        for i in range(warmup + reps):
            ctx.enqueue_steps(64)
            ctx.sync()
            if i >= warmup:
                single.append(ctx.last_run_ms() * 1000 / 64)
        kernel = ctx.launch_info()["kernel"].split("<")[0]
        s = statistics.median(single)
        per_radius = {}
        for radius in radii:
            ctx.init_disk(n // 2, n // 2, n // 3, 1.0, -1.0)
            t = []
            for i in range(warmup + reps):
                assert capi.localized_run(ctx, radius, 64)[0] == 64
                if i >= warmup:
                    t.append(ctx.last_run_ms() * 1000 / 64)
            per_radius[radius] = statistics.median(t)
            rows.append({"probe": "localized-cost", "n": n, "channels": channels, "radius": radius, "clock": "HIP events around 64 iterations",
                         "reps": reps, "warmup": warmup, "iteration_us": round(per_radius[radius], 2), "min_max_us": [round(min(t), 2), round(max(t), 2)],
                         "two_phase_iteration_us": round(s, 2), "two_phase_kernel": kernel, "ratio_to_two_phase": round(per_radius[radius] / s, 3),
                         "strip_rows": capi.localized_geometry(n, n, radius)[3], "bytes_per_pixel_iteration": 48 + 30 * channels,
                         "GB_per_s_by_those_bytes": round((48 + 30 * channels) * n * n / per_radius[radius] / 1e3, 1)})
        if len(radii) > 1:
            rows.append({"probe": "localized-radius-ratio", "n": n, "channels": channels, "radii": [max(radii), min(radii)],
                         "ratio": round(per_radius[max(radii)] / per_radius[min(radii)], 3)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["1024x1", "2048x1", "4096x1", "4096x3"], help="side x channels")
    ap.add_argument("--radii", nargs="+", type=int, default=[2, 10, 32, 127])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=150, help="seconds a plane's child process may take")
    ap.add_argument("--case", default="", help="(child) one plane, rows to stdout")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.case:
        n, ch = (int(x) for x in args.case.split("x"))
        for r in cost(n, ch, args.radii, args.reps, args.warmup):
            print(json.dumps(r), flush=True)
        return 0
    lines, status = [], 0
    for case in args.cases:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps),
               "--warmup", str(args.warmup), "--radii", *[str(r) for r in args.radii]]
        out = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(out.stdout)
        sys.stdout.flush()
        lines += [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        status = out.returncode
        if status != 0:   # a fault, an abort or the time limit: nothing more is started on the device
            sys.stderr.write(out.stderr[-4000:])
            print(f"{case}: exit status {status}; the probe ends here", file=sys.stderr)
            break
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if lines and status == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
