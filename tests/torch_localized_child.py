"""Child process of test_gpu_torch_localized.py: torch first, then the library -- one HIP runtime.  Segmenter(localized=R) on two 64 x 64
device tensors returns the masks of the capi path (contexts fed the same inputs call for call, capi.localized_run) byte for byte, from
an Otsu start and from a disk start; what does not compose is refused; the default path gives what contexts of their own give with
Context.run.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, torch_io  # noqa: E402
import localized_util as L  # noqa: E402

N, H, W, STEPS, RADIUS = 2, 64, 64, 12, 6


def main():
    imgs = np.stack([L.scene(H, W, 1, seed=5 + i)[0][0] for i in range(N)])
    dev = torch.from_numpy(imgs).cuda()
    params = capi.make_params(tol=0.0, mu=20.0)
    disk = ("disk", [(32, 32, 20)] * N)
    with torch_io.Segmenter(N, H, W, 1, params=params, localized=RADIUS) as seg:
        assert seg.localized == RADIUS
        results = {}
        for name, init in (("otsu", "otsu"), ("disk", disk)):
            masks, steps, norms = seg.segment(dev, STEPS, init=init)
            assert masks.dtype == torch.uint8 and tuple(masks.shape) == (N, H, W) and steps == [STEPS] * N and np.isfinite(norms).all()
            results[name] = (masks.cpu().numpy(), seg.levelsets().cpu().numpy(), norms)
            assert seg.components()[1] == [c.components(cap=0)[0] for c in seg.contexts]   # everything after the run is unchanged
        for bad in (dict(reinit_every=4), dict(energy_every=4)):
            try:
                seg.segment(dev, STEPS, **bad)
            except ValueError:
                continue
            raise AssertionError(bad)
    for i in range(N):
        for name, start in (("otsu", lambda c: c.init_otsu()), ("disk", lambda c: c.init_disk(32, 32, 20, 1.0, 0.0))):
            with capi.Context(H, W, 1, params) as ctx:
                ctx.set_image([imgs[i]])
                start(ctx)
                done, nrm, _ = capi.localized_run(ctx, RADIUS, STEPS)
                got_m, got_u, norms = results[name]
                assert done == STEPS and nrm == norms[i]
                assert np.array_equal(ctx.get_mask(), got_m[i])
                assert np.array_equal(ctx.get_levelset().view(np.uint64), got_u[i].view(np.uint64))
    # the default takes none of the new branches: the two-phase run of contexts of their own, bit for bit
    with torch_io.Segmenter(N, H, W, 1, params=params) as seg:
        masks, steps, norms = seg.segment(dev, STEPS)
        assert seg.localized is None and steps == [STEPS] * N
        u = seg.levelsets().cpu().numpy()
        for i in range(N):
            with capi.Context(H, W, 1, params) as ctx:
                ctx.set_image([imgs[i]])
                ctx.init_checkerboard()
                assert ctx.run(STEPS) == (STEPS, norms[i])
                assert np.array_equal(ctx.get_levelset().view(np.uint64), u[i].view(np.uint64))
                assert np.array_equal(ctx.get_mask(), masks[i].cpu().numpy())
    for bad in (dict(localized=0), dict(localized=128), dict(localized=True), dict(localized=2.0), dict(localized=3, phases=4),
                dict(localized=3, levels=2)):
        try:
            torch_io.Segmenter(N, H, W, 1, **bad)
        except ValueError:
            continue
        raise AssertionError(bad)
    print("torch_localized child ok")


if __name__ == "__main__":
    main()
