"""Child process of test_gpu_reinit.py (one fresh process per case, so that each GPU leg runs under the parent's time limit).
  torch            Segmenter.segment(reinit_every=20) against capi.run_batch_with_reinit's loop on host-fed contexts (torch first: one
                   HIP runtime, capi.py's rule)
  fullsize disk    4096 x 4096, the BASELINE disk (synth.config_planes("C2")) after 50 iterations from the checkerboard
  fullsize noisy   4096 x 4096, a noisy disk after 20
Exits non-zero on the first mismatch; prints every figure before it asserts."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_case():
    import torch  # noqa: F401  (before chan_vese_amd)
    from chan_vese_amd import capi, synth, torch_io
    N, H, W, STEPS, EVERY = 6, 128, 160, 50, 20
    imgs = np.stack([synth.disk(H, 200 - 6 * i, 40 + 5 * i, noise=16, seed=40 + i, h=H, w=W) for i in range(N)])
    host = [capi.Context(H, W, 1) for _ in range(N)]
    for ctx, img in zip(host, imgs):
        ctx.set_option("co_resident", 0)
        ctx.set_image([img])
        ctx.init_checkerboard()
    want_res = capi.run_batch_with_reinit(host, STEPS, EVERY)
    want = np.stack([ctx.get_mask() for ctx in host])
    with torch_io.Segmenter(N, H, W, 1, options={"co_resident": 0}) as seg:
        t = torch.from_numpy(imgs).cuda()
        masks, steps, norms = seg.segment(t, STEPS, reinit_every=EVERY)
        print("steps", steps, "want", [r[0] for r in want_res])
        assert list(zip(steps, norms)) == want_res
        assert np.array_equal(masks.cpu().numpy(), want)
        for i in (0, N - 1):
            assert np.array_equal(seg.levelsets()[i].cpu().numpy().view(np.uint64), host[i].get_levelset().view(np.uint64))
        # reinit_every = 0 is today's segment()
        plain, steps0, norms0 = seg.segment(t, STEPS)
        again, steps1, norms1 = seg.segment(t, STEPS, reinit_every=0)
        assert np.array_equal(plain.cpu().numpy(), again.cpu().numpy()) and (steps0, norms0) == (steps1, norms1)
    for ctx in host:
        ctx.close()
    print("reinit child ok: torch")


def fullsize_case(case):
    from chan_vese_amd import capi, synth
    import reinit_util as R
    n = 4096
    planes, steps = (synth.config_planes("C2"), 50) if case == "disk" else ([synth.disk(n, 200, 50, noise=48, seed=77)], 20)
    with capi.Context(n, n, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image(planes)
        ctx.init_checkerboard()
        done, _ = ctx.run(steps)
        assert done == steps
        before, mask0 = ctx.get_levelset(), ctx.get_mask()
        t0 = time.time()
        changed = ctx.reinit()
        t1 = time.time()
        after, mask1 = ctx.get_levelset(), ctx.get_mask()
    print(f"{case}: reinit of 4096^2 took {1e3 * (t1 - t0):.2f} ms of host time (first call: workspace allocation included), changed={changed}")
    assert changed
    rows = np.unique(np.concatenate([[0, n - 1], np.random.default_rng(20261017).choice(np.arange(1, n - 1), 14, replace=False)]))
    assert len(rows) == 16
    d2, want, _ = R.signed_edt(before, rows=rows)
    print(f"{case}: rows {rows.tolist()}, max d2 in them {int(d2.max())} (distance {np.sqrt(float(d2.max())):.1f})")
    if case == "disk":                                                     # the worst case it is named for: four-digit distances
        assert d2.max() >= 1000 ** 2, "the disk's level set no longer has long searches in the compared rows"
    for r, i in enumerate(rows):                                           # every listed row, none skipped
        bad = int((R.bits(after[i]) != R.bits(want[r])).sum())
        print(f"{case}: row {i}: {bad} differing values")
        assert bad == 0
    packed0, packed1 = np.packbits(mask0), np.packbits(mask1)
    assert np.array_equal(packed0, np.packbits(R.mask_of(before))) and np.array_equal(packed1, packed0)
    assert np.array_equal(np.packbits(R.mask_of(after)), packed0) and np.abs(after).min() >= 0.5
    print(f"reinit child ok: fullsize {case}")


if __name__ == "__main__":
    if sys.argv[1] == "torch":
        torch_case()
    else:
        fullsize_case(sys.argv[2])
