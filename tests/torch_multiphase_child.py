"""Child process of test_gpu_torch_multiphase.py: torch first, then the library -- one HIP runtime.  Segmenter(phases=4) on two 64 x 64
device tensors: the labels are mask_A + 2 mask_B of phase_masks(), and equal the capi path (contexts fed the same inputs call for call,
capi.multiphase_run, Context.multiphase_labels_with) byte for byte; the post-processing methods take phase = 0 | 1; phases = 2 refuses
what belongs to four phases.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, torch_io  # noqa: E402
import multiphase_util as M  # noqa: E402

N, H, W, STEPS = 2, 64, 64, 12


def main():
    imgs = np.stack([M.disks_image(H, W, 1, noise=4.0 + 4 * i, seed=11 + i)[0][0] for i in range(N)])
    dev = torch.from_numpy(imgs).cuda()
    params = capi.make_params(tol=0.0)
    with torch_io.Segmenter(N, H, W, 1, params=params, phases=4) as seg:
        labels, steps, norms = seg.segment(dev, STEPS)
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (N, H, W) and int(labels.max()) <= 3
        assert steps == [STEPS] * N and all(len(n) == 2 and np.isfinite(n).all() for n in norms)
        ma, mb = seg.phase_masks()
        assert torch.equal(labels, ma + 2 * mb)
        got = labels.cpu().numpy()
        u = [seg.levelsets(phase=p).cpu().numpy() for p in (0, 1)]
        assert not np.array_equal(u[0], u[1])
        for i in range(N):
            assert np.array_equal(got[i], M.labels(u[0][i], u[1][i]))
        # the post-processing methods on either phase: the contexts' own answers
        for p, ctxs in ((0, seg.contexts), (1, seg.contexts_b)):
            lab, counts = seg.components(phase=p)
            assert counts == [c.components(cap=0)[0] for c in ctxs]
            assert torch.equal(seg.clean_masks(phase=p), (ma, mb)[p])
        for bad in (dict(phase=2), dict(phase=True)):
            try:
                seg.components(**bad)
            except ValueError:
                continue
            raise AssertionError(bad)
        for bad in (dict(invert=True), dict(reinit_every=4), dict(energy_every=4), dict(init=("mask", ma))):
            try:
                seg.segment(dev, STEPS, **bad)
            except ValueError:
                continue
            raise AssertionError(bad)
        # another second start: Otsu for phi2
        labels2, _, _ = seg.segment(dev, STEPS, init2="otsu")
        assert not torch.equal(labels2, labels)
    # the capi path: contexts of their own, the same calls
    cb = capi.checkerboard_host(H, W)
    for i in range(N):
        with capi.Context(H, W, 1, params) as a, capi.Context(H, W, 1, params) as b:
            a.set_image([imgs[i]])
            b.set_image([imgs[i]])
            a.init_checkerboard()
            b.set_levelset(np.roll(cb, (2, 3), axis=(0, 1)))
            done, nrm, _ = capi.multiphase_run(a, b, STEPS)
            assert done == STEPS and nrm == norms[i]
            assert np.array_equal(a.multiphase_labels_with(b), got[i])
            assert np.array_equal(a.get_levelset().view(np.uint64), u[0][i].view(np.uint64))
            assert np.array_equal(b.get_levelset().view(np.uint64), u[1][i].view(np.uint64))
    # phases = 2 is the plain path and refuses what belongs to four phases
    with torch_io.Segmenter(N, H, W, 1, params=params) as seg:
        masks, steps, _ = seg.segment(dev, STEPS)
        assert masks.dtype == torch.uint8 and steps == [STEPS] * N and seg.phases == 2 and seg.contexts_b == []
        for call in (lambda: seg.segment(dev, STEPS, init2="otsu"), lambda: seg.phase_masks(), lambda: seg.components(phase=1)):
            try:
                call()
            except ValueError:
                continue
            raise AssertionError("phases = 2 took a four-phase argument")
    for bad in (dict(phases=3), dict(phases=4, levels=2), dict(phases=4, local=(2, "mean")), dict(phases=2, params2=params)):
        try:
            torch_io.Segmenter(N, H, W, 1, **bad)
        except ValueError:
            continue
        raise AssertionError(bad)
    print("torch_multiphase child ok")


if __name__ == "__main__":
    main()
