#!/usr/bin/env python3
"""What does cvh_localized_run_batch / cvh_multiphase_run_batch buy over a loop of the single calls?  Records, asserts nothing.

Per shape (N x side^2: 64 x 256^2, 32 x 512^2, 8 x 1024^2, 2 x 2048^2), channel count (1, 3) and flow (localised at R = 2 and R = 10,
four-phase pairs): N members run 64 iterations (tol = 0, "sync_every" 64) through ONE batch call and through a loop of N single calls,
in one process, 20 timed rounds after 3, the two ways alternating.  Reported per way: us per member-iteration by the host's clock
around the call(s) -- a call ends with its host wait, so this is what a caller sees -- and by the device's (cvh_last_run_ms: of member
0 for the batch, summed over the members for the loop; the gaps between the loop's calls are not in it), the medians, and the ratio
loop / batch of each clock.

Every shape runs in a child process of its own under a time limit; the first child that fails ends the probe.

    python tools/march_batch_probe.py [--cases 64x256 32x512 8x1024 2x2048] [--channels 1 3] [--radii 2 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERATIONS = 64


def members(capi, synth, count, side, channels, params):
    out = []
    for i in range(count):
        ctx = capi.Context(side, side, channels, params)
        ctx.set_image([synth.disk(side, 180 - 60 * k, 40 + 80 * k, noise=16, seed=7 + k + 3 * i) for k in range(channels)])
        ctx.set_option("sync_every", ITERATIONS)
        out.append(ctx)
    return out


def timed(rounds, warmup, ways, prepare):
    """ways: {name: callable returning the device's ms}; alternating, prepare() -- the members' start, outside the clock -- in front of
    each, the first `warmup` rounds dropped -> {name: (host us, device us)}"""
    host, dev = {k: [] for k in ways}, {k: [] for k in ways}
    for i in range(warmup + rounds):
        for name, call in ways.items():
            prepare()
            t0 = time.perf_counter()
            ms = call()
            t1 = time.perf_counter()
            if i >= warmup:
                host[name].append((t1 - t0) * 1e6)
                dev[name].append(ms * 1e3)
    return {k: (host[k], dev[k]) for k in ways}


def row(flow, count, side, channels, radius, res, reps, warmup):
    per = count * ITERATIONS
    med = {k: (statistics.median(v[0]) / per, statistics.median(v[1]) / per) for k, v in res.items()}
    return {"probe": "march-batch", "flow": flow, "members": count, "n": side, "channels": channels, "radius": radius, "iterations": ITERATIONS,
            "reps": reps, "warmup": warmup, "clock": "host perf_counter around the call(s); device: cvh_last_run_ms",
            "batch_us_per_member_iteration": round(med["batch"][0], 3), "loop_us_per_member_iteration": round(med["loop"][0], 3),
            "ratio_loop_over_batch": round(med["loop"][0] / med["batch"][0], 3),
            "batch_device_us": round(med["batch"][1], 3), "loop_device_us": round(med["loop"][1], 3),
            "device_ratio_loop_over_batch": round(med["loop"][1] / med["batch"][1], 3),
            "batch_host_min_max_us": [round(min(res["batch"][0]) / per, 3), round(max(res["batch"][0]) / per, 3)],
            "loop_host_min_max_us": [round(min(res["loop"][0]) / per, 3), round(max(res["loop"][0]) / per, 3)]}


def cost(count, side, channel_counts, radii, reps, warmup):
    from chan_vese_amd import capi, synth
    rows = []
    for channels in channel_counts:
        ctxs = members(capi, synth, count, side, channels, capi.make_params(tol=0.0, mu=100.0))
        try:
            for radius in radii:
                def start():
                    capi.init_disk_batch(ctxs, [(side // 2, side // 2, side // 3)] * count)
                    ctxs[0].sync()

                def batch():
                    assert all(r[0] == ITERATIONS for r in capi.localized_run_batch(ctxs, radius, ITERATIONS))
                    return ctxs[0].last_run_ms()

                def loop():
                    ms = 0.0
                    for c in ctxs:
                        assert capi.localized_run(c, radius, ITERATIONS)[0] == ITERATIONS
                        ms += c.last_run_ms()
                    return ms
                rows.append(row("localized", count, side, channels, radius, timed(reps, warmup, {"batch": batch, "loop": loop}, start), reps, warmup))
                print(json.dumps(rows[-1]), flush=True)
        finally:
            for c in ctxs:
                c.close()
        a = members(capi, synth, count, side, channels, capi.make_params(tol=0.0))
        b = members(capi, synth, count, side, channels, capi.make_params(tol=0.0))
        try:
            def start2():
                capi.init_checkerboard_batch(a)
                capi.init_disk_batch(b, [(side // 2, side // 2, side // 3)] * count)
                a[0].sync()
                b[0].sync()

            def batch2():
                assert all(r[0] == ITERATIONS for r in capi.multiphase_run_batch(list(zip(a, b)), ITERATIONS))
                return a[0].last_run_ms()

            def loop2():
                ms = 0.0
                for x, y in zip(a, b):
                    assert capi.multiphase_run(x, y, ITERATIONS)[0] == ITERATIONS
                    ms += x.last_run_ms()
                return ms
            rows.append(row("multiphase", count, side, channels, None, timed(reps, warmup, {"batch": batch2, "loop": loop2}, start2), reps, warmup))
            print(json.dumps(rows[-1]), flush=True)
        finally:
            for c in a + b:
                c.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["64x256", "32x512", "8x1024", "2x2048"], help="members x side")
    ap.add_argument("--channels", nargs="+", type=int, default=[1, 3])
    ap.add_argument("--radii", nargs="+", type=int, default=[2, 10])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--case", default="", help="(child) one shape, rows to stdout")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.case:
        count, side = (int(x) for x in args.case.split("x"))
        cost(count, side, args.channels, args.radii, args.reps, args.warmup)
        return 0
    lines, status = [], 0
    for case in args.cases:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps),
               "--warmup", str(args.warmup), "--radii", *[str(r) for r in args.radii], "--channels", *[str(c) for c in args.channels]]
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
