"""Child process of test_gpu_torch_pyramid.py: torch first, then the library -- one HIP runtime.  Segmenter(levels=3).segment on
3 x 64 x 144 against capi.run_coarse_to_fine_batch on contexts of the same options, and levels=1 against the plain Segmenter.
Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, synth, torch_io  # noqa: E402

N, H, W, LEVELS, STEPS = 3, 64, 144, 3, 40
OPTIONS = {"wave_pol": 0}   # (batch members never take the resident flow; the cache policy is the one choice that weighs neighbours)


def main():
    imgs = np.stack([synth.disk(H, 200 - 20 * i, 40 + 15 * i, noise=16, seed=50 + i, h=H, w=W) for i in range(N)])
    t = torch.from_numpy(imgs).cuda()
    shapes = capi.pyramid_shapes(H, W, LEVELS)
    host = [[capi.Context(h, w, 1) for h, w in shapes] for _ in range(N)]
    for pyr in host:
        for ctx in pyr:
            ctx.set_option("wave_pol", 0)
    with torch_io.Segmenter(N, H, W, 1, options=OPTIONS, levels=LEVELS) as seg:
        assert len(seg.pyramids) == N and all(len(p) == LEVELS for p in seg.pyramids) and seg.contexts == [p[0] for p in seg.pyramids]
        for init, start in (("checkerboard", lambda cs: capi.init_checkerboard_batch(cs)), ("otsu", lambda cs: capi.init_otsu_batch(cs)),
                            (("disk", (72, 32, 24)), lambda cs: capi.init_disk_batch(cs, (72 >> 2, 32 >> 2, 24 >> 2))),
                            (("rect", (30, 10, 80, 40)), lambda cs: capi.init_rect_batch(cs, (30 >> 2, 10 >> 2, 80 >> 2, 40 >> 2)))):
            for pm in (None, (30.0, 0.25, 1.0)):
                if pm and init != "otsu":
                    continue
                for i, pyr in enumerate(host):
                    pyr[0].set_image([imgs[i]])
                if pm:
                    capi.perona_malik_batch([p[0] for p in host], *pm)
                for k in range(LEVELS - 1):
                    capi.restrict_image_batch([p[k] for p in host], [p[k + 1] for p in host])
                start([p[-1] for p in host])
                want = capi.run_coarse_to_fine_batch(host, STEPS)
                masks, steps, norms = seg.segment(t, STEPS, perona_malik=pm, init=init)
                assert seg.level_steps == [[r[0] for r in m] for m in want], (init, seg.level_steps, want)
                assert list(zip(steps, norms)) == [m[0] for m in want], init
                for i, pyr in enumerate(host):
                    assert np.array_equal(masks[i].cpu().numpy(), pyr[0].get_mask()), (init, i)
                    assert np.array_equal(seg.levelsets()[i].cpu().numpy().view(np.uint64), pyr[0].get_levelset().view(np.uint64)), (init, i)
        for bad in (dict(init=torch.zeros((N, H, W), dtype=torch.float64).cuda()), dict(reinit_every=4)):
            try:
                seg.segment(t, STEPS, **bad)
            except ValueError:
                continue
            raise AssertionError(f"levels = 3 accepted {list(bad)}")
    for pyr in host:
        for ctx in pyr:
            ctx.close()
    # levels = 1 is the plain path: the same bytes
    with torch_io.Segmenter(N, H, W, 1, options={"co_resident": 0}, levels=1) as a, torch_io.Segmenter(N, H, W, 1, options={"co_resident": 0}) as b:
        ra, rb = a.segment(t, STEPS, init="otsu"), b.segment(t, STEPS, init="otsu")
        assert ra[1:] == rb[1:] and torch.equal(ra[0], rb[0]) and a.level_steps is None
        assert torch.equal(a.levelsets().view(torch.int64), b.levelsets().view(torch.int64))
    print("torch_pyramid child ok")


if __name__ == "__main__":
    main()
