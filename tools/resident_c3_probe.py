"""Three channels: the resident flow ("resident" = 1, csv_resident_kernel<3, NRT>) against the per-launch flow ("resident" = 0) in ONE
process, one context per size, the two flows ALTERNATED in that context, in both orders: HIP-event time per iteration
(cvh_last_run_ms) of STEPS iterations from the checkerboard on a noisy three-colour disk.  The per-launch flow is the one this build
shares with every build before the three-channel resident kernel existed.  The last block repeats the pair for ONE channel at 2048^2
(the one-channel resident kernel's instructions did not change: the figure belongs beside the 12.0-12.2 us on record).
usage: resident_c3_probe.py  [SIZES=256x256,512x512,1024x1024,1080x1920,1536x2048 STEPS=400 ALTS=4 C1=2048x2048]"""
import os, sys
sys.path.insert(0, '.')
import numpy as np
from chan_vese_amd import capi, synth

steps = int(os.environ.get("STEPS", "400")); alts = int(os.environ.get("ALTS", "4"))
sizes = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("SIZES", "256x256,512x512,1024x1024,1080x1920,1536x2048").split(",") if s]
c1_sizes = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("C1", "2048x2048").split(",") if s]


def colour_disk(h, w):
    n = max(h, w)
    return [synth.disk(n, fg, bg, noise=20, seed=31 + k, h=h, w=w) for k, (fg, bg) in enumerate(((200, 50), (90, 160), (230, 120)))]


def one_size(h, w, channels):
    planes = colour_disk(h, w)[:channels]
    pk = dict(tol=0.0)
    if channels == 3: pk.update(lambda1=[1, 0.8, 0.5], lambda2=[0.7, 0.5, 1])
    with capi.Context(h, w, channels, capi.make_params(**pk)) as ctx:
        ctx.set_image(planes)
        t = {1: [], 0: []}
        kernels = {}
        for flow in (1, 0):                               # warm both flows: code objects, graphs, buffers
            ctx.set_option("resident", flow); ctx.init_checkerboard()
            ctx.warm(steps); ctx.enqueue_steps(steps); ctx.sync()
            kernels[flow] = ctx.launch_info()["kernel"]
        for alt in range(alts):
            for flow in ((1, 0) if alt % 2 == 0 else (0, 1)):   # both orders
                ctx.set_option("resident", flow); ctx.init_checkerboard()
                ctx.warm(steps); ctx.enqueue_steps(steps)
                done = ctx.sync()[0]
                assert done == steps, (h, w, flow, done)
                t[flow].append(ctx.last_run_ms() * 1e3 / steps)
        r, p = np.array(t[1]), np.array(t[0])
        print("%5d x %4d x%d  resident %6.2f us (%.2f-%.2f)  per launch %6.2f us (%.2f-%.2f)  ratio %.3f   [%s | %s]   resident: %s   per launch: %s" % (
            h, w, channels, np.median(r), r.min(), r.max(), np.median(p), p.min(), p.max(), np.median(r) / np.median(p), kernels[1], kernels[0],
            " ".join("%.2f" % v for v in r), " ".join("%.2f" % v for v in p)), flush=True)


print("us per iteration, %d iterations from the checkerboard, %d alternations (median (min-max)); ratio = resident / per launch" % (steps, alts), flush=True)
for h, w in sizes: one_size(h, w, 3)
for h, w in c1_sizes: one_size(h, w, 1)
