"""Wave timeline of ONE iteration of a batch of contexts, fused (cvh_enqueue_steps_batch) or interleaved on their own streams: per-wave
start / end stamps (option "debug_times", 100 MHz realtime, one clock for the whole device), where the waves ran (XCD, SE, CU), and
so how the iteration's time splits into body and tail and how evenly the workgroups fill the CUs.
usage: fused_batch_timeline.py  [CASE=8x4096x4096 MODE=fused|interleaved STRIP_ROWS=0 (auto) WARM=32]"""
import ctypes as C, os, sys
sys.path.insert(0, '.')
import numpy as np
from chan_vese_amd import capi, synth

count, h, w = (int(v) for v in os.environ.get("CASE", "8x4096x4096").split("x"))
mode = os.environ.get("MODE", "fused"); strip_rows = int(os.environ.get("STRIP_ROWS", "0")); warm = int(os.environ.get("WARM", "32"))
L = capi.lib()
L.cvh_debug_read.restype = C.c_int
L.cvh_debug_read.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_long, C.POINTER(C.c_long), C.POINTER(C.c_int)]

ctxs = []
for b in range(count):
    ctx = capi.Context(h, w, 1, capi.make_params(tol=0.0))
    ctx.set_option("resident", 0)
    if strip_rows: ctx.set_option("strip_rows", strip_rows)
    r = min(h, w) // 4 + 4 * (b % 8) - 14
    ctx.set_image([synth.disk(min(h, w), 200, 50, noise=16, seed=1000 + b, radius=r, h=h, w=w)])
    ctx.init_checkerboard()
    ctxs.append(ctx)


def iterate(n):
    if mode == "fused":
        capi.enqueue_steps_batch(ctxs, n)
    else:
        for ctx in ctxs: ctx.enqueue_steps(n)
    for ctx in ctxs: ctx.sync()


iterate(warm)
for ctx in ctxs: ctx.set_option("debug_times", 1)     # fresh (zeroed) stamp buffers: only the next iteration's stamps
iterate(1)

rows = []   # start, end, member, block, cu key
for m, ctx in enumerate(ctxs):
    buf = np.zeros(4_000_000, dtype=np.uint64); words = C.c_long(0); nb = C.c_int(0)
    L.cvh_debug_read(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint64)), buf.size, C.byref(words), C.byref(nb))
    nb = nb.value
    rec = buf[:nb * 16].reshape(nb * 4, 4)
    for i in np.nonzero(rec[:, 1] > 0)[0]:
        d3 = int(rec[i, 3]); hw = (d3 >> 8) & 0xffffffff
        cu = (d3 & 0xff, (hw >> 13) & 0x7, (hw >> 12) & 1, (hw >> 8) & 0xf)   # XCD, SE, SH, CU
        rows.append((int(rec[i, 0]), int(rec[i, 1]), m, i // 4, cu))
t0 = min(r[0] for r in rows)
st = np.array([(r[0] - t0) / 100.0 for r in rows]); en = np.array([(r[1] - t0) / 100.0 for r in rows])
print("%d x %dx%d  %s  strip_rows %s  kernel %s" % (count, h, w, mode, strip_rows or "auto", ctxs[0].launch_info()["kernel"]))
print("waves stamped %d in %d workgroups; iteration span %.2f us (first wave start -> last wave end)"
      % (len(rows), len({(r[2], r[3]) for r in rows}), en.max()))
print("wave start us: p50 %.2f p90 %.2f max %.2f" % (np.median(st), np.percentile(st, 90), st.max()))
print("wave end   us: p10 %.2f p50 %.2f p90 %.2f p99 %.2f max %.2f" % tuple(np.percentile(en, [10, 50, 90, 99, 100])))
print("wave dur   us: p10 %.2f p50 %.2f max %.2f" % tuple(np.percentile(en - st, [10, 50, 100])))
per_cu = {}
for r, e in zip(rows, en):
    wgs, last = per_cu.get(r[4], (set(), 0.0))
    wgs.add((r[2], r[3])); per_cu[r[4]] = (wgs, max(last, e))
hist = {}
for wgs, _ in per_cu.values(): hist[len(wgs)] = hist.get(len(wgs), 0) + 1
last = np.array([v[1] for v in per_cu.values()])
print("CUs used %d; workgroups per CU: %s" % (len(per_cu), ", ".join("%d: %d CUs" % (k, hist[k]) for k in sorted(hist))))
print("last wave end per CU us: min %.2f p10 %.2f p50 %.2f max %.2f  (the tail: CUs idle from their last end to the iteration's)" % tuple(np.percentile(last, [0, 10, 50, 100])))
for m in range(min(count, 8)):
    sel = np.array([r[2] == m for r in rows])
    print("  member %d: waves %5d  start %.2f .. %.2f  end %.2f .. %.2f us" % (m, sel.sum(), st[sel].min(), st[sel].max(), en[sel].min(), en[sel].max()))
for ctx in ctxs: ctx.close()
