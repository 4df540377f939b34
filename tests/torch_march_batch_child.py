"""Child process of test_gpu_torch_march_batch.py: torch first, then the library -- one HIP runtime.  Segmenter(localized=R) and
Segmenter(phases=4) on three 40 x 70 device tensors call the batch forms (checked: the single wrappers are not entered); masks, labels,
level sets, steps and norms equal capi.localized_run / capi.multiphase_run on contexts of their own fed the same inputs, bit for bit.
Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, torch_io  # noqa: E402
import localized_util as L  # noqa: E402
import multiphase_util as M  # noqa: E402

N, H, W, STEPS, RADIUS = 3, 40, 70, 7, 5


def counted(name, calls):
    real = getattr(capi, name)

    def wrapper(*a, **k):
        calls.append(name)
        return real(*a, **k)
    setattr(capi, name, wrapper)
    return real


def main():
    calls = []
    real = {name: counted(name, calls) for name in ("localized_run", "multiphase_run", "localized_run_batch", "multiphase_run_batch")}
    # ---- localised
    imgs = np.stack([L.scene(H, W, 1, seed=5 + i)[0][0] for i in range(N)])
    dev = torch.from_numpy(imgs).cuda()
    params = capi.make_params(tol=0.0, mu=20.0)
    with torch_io.Segmenter(N, H, W, 1, params=params, localized=RADIUS) as seg:
        masks, steps, norms = seg.segment(dev, STEPS, init="otsu")
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == (N, H, W) and steps == [STEPS] * N and len(norms) == N
        got_m, got_u = masks.cpu().numpy(), seg.levelsets().cpu().numpy()
    assert calls == ["localized_run_batch"], calls
    for i in range(N):
        with capi.Context(H, W, 1, params) as ctx:
            ctx.set_image([imgs[i]])
            ctx.init_otsu()
            done, nrm, _ = real["localized_run"](ctx, RADIUS, STEPS)
            assert done == STEPS and nrm == norms[i]
            assert np.array_equal(ctx.get_mask(), got_m[i])
            assert np.array_equal(ctx.get_levelset().view(np.uint64), got_u[i].view(np.uint64))
    # ---- four phases
    del calls[:]
    imgs = np.stack([M.disks_image(H, W, 1, noise=4.0 + 4 * i, seed=11 + i)[0][0] for i in range(N)])
    dev = torch.from_numpy(imgs).cuda()
    params = capi.make_params(tol=0.0)
    with torch_io.Segmenter(N, H, W, 1, params=params, phases=4) as seg:
        labels, steps, norms = seg.segment(dev, STEPS)
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (N, H, W) and steps == [STEPS] * N
        assert all(len(n) == 2 for n in norms)
        got = labels.cpu().numpy()
        u = [seg.levelsets(phase=p).cpu().numpy() for p in (0, 1)]
    assert calls == ["multiphase_run_batch"], calls
    cb = capi.checkerboard_host(H, W)
    for i in range(N):
        with capi.Context(H, W, 1, params) as a, capi.Context(H, W, 1, params) as b:
            a.set_image([imgs[i]])
            b.set_image([imgs[i]])
            a.init_checkerboard()
            b.set_levelset(np.roll(cb, (2, 3), axis=(0, 1)))
            done, nrm, _ = real["multiphase_run"](a, b, STEPS)
            assert done == STEPS and tuple(nrm) == tuple(norms[i])
            assert np.array_equal(a.multiphase_labels_with(b), got[i])
            assert np.array_equal(a.get_levelset().view(np.uint64), u[0][i].view(np.uint64))
            assert np.array_equal(b.get_levelset().view(np.uint64), u[1][i].view(np.uint64))
    print("torch_march_batch child ok")


if __name__ == "__main__":
    main()
