"""Child process of test_gpu_torch_energy.py: torch first, then the library -- one HIP runtime.  Segmenter.energies() after segment() on
3 x 48 x 80 device tensors equals Context.energy() of contexts fed the same inputs call for call, bit for bit, and of the segmenter's own
contexts; segment(energy_every=K) stores the series run_batch_monitored returns and leaves the masks of a plain segment().  Exits
non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, synth, torch_io  # noqa: E402

N, H, W, STEPS, EVERY = 3, 48, 80, 40, 16
OPTIONS = {"wave_pol": 0}   # (batch members never take the resident flow; the cache policy is the one choice that weighs neighbours)
FIELDS = ("total", "length", "area", "fit_in", "fit_out", "c1", "c2")


def same(a, b):
    return all(np.array_equal(np.asarray(getattr(a, f), dtype=np.float64).view(np.uint64), np.asarray(getattr(b, f), dtype=np.float64).view(np.uint64))
               for f in FIELDS)


def main():
    imgs = np.stack([synth.disk(64, 200, 50, noise=8 + 4 * i, seed=3 + i, h=H, w=W) for i in range(N)])
    dev = torch.from_numpy(imgs).cuda()
    params = capi.make_params(tol=0.0)
    with torch_io.Segmenter(N, H, W, 1, params=params, options=OPTIONS) as seg:
        masks, steps, _ = seg.segment(dev, STEPS)
        assert steps == [STEPS] * N and seg.energy_series is None
        got = seg.energies()
        assert all(same(g, c.energy()) for g, c in zip(got, seg.contexts))
        plain = masks.cpu().numpy()
    # contexts of their own, the same calls: set_image, checkerboard, run_batch
    ctxs = [capi.Context(H, W, 1, params) for _ in range(N)]
    try:
        for c, img in zip(ctxs, imgs):
            c.set_option("wave_pol", 0)
            c.set_image([img])
        capi.init_checkerboard_batch(ctxs)
        capi.run_batch(ctxs, STEPS)
        for i, c in enumerate(ctxs):
            assert same(got[i], c.energy()), (i, got[i], c.energy())
    finally:
        for c in ctxs:
            c.close()
    with torch_io.Segmenter(N, H, W, 1, params=params, options=OPTIONS) as seg:
        masks, steps, _ = seg.segment(dev, STEPS, energy_every=EVERY)
        assert steps == [STEPS] * N
        for i, series in enumerate(seg.energy_series):
            assert [s for s, _ in series] == [16, 32, 40]
            assert same(series[-1][1], seg.energies()[i])
            tot = [e.total for _, e in series]
            assert all(b < a for a, b in zip(tot, tot[1:])), tot
            assert abs(tot[-1] - got[i].total) <= 1e-9 * abs(got[i].total)
        assert np.array_equal(masks.cpu().numpy(), plain)
        for bad in (dict(energy_every=-1), dict(energy_every=2.0), dict(energy_every=8, reinit_every=8)):
            try:
                seg.segment(dev, STEPS, **bad)
            except ValueError:
                continue
            raise AssertionError(bad)
    print("torch_energy child ok")


if __name__ == "__main__":
    main()
