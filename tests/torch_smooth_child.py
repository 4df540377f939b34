"""Child process of test_gpu_torch_smooth.py: torch first, then the library -- one HIP runtime.  On device tensors of 64 x 64:
Segmenter(smooth=(1.5, "blur")) reports images() equal to the restatement (smooth_util) and the masks of the capi sequence (set_image,
smooth_planes_to, the start, run, get_mask); behind rank= and in front of local= the stages run in that order; with edge=K,
edge_sigma=2 the edge planes are the numpy edge map (geodesic_util) of the BLURRED planes while images() are still the unblurred ones,
and masks, norms and level sets are those of the capi sequence (smooth_planes_to a scratch context, edge_map_from it, geodesic_run).
Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, torch_io  # noqa: E402
import geodesic_util as G  # noqa: E402
import local_util as LU  # noqa: E402
import rank_util as RU  # noqa: E402
import smooth_util as U  # noqa: E402

N, H, W, STEPS, K = 2, 64, 64, 12, 15.0
OPTIONS = {"wave_pol": 0}   # (batch members never take the resident flow; the cache policy is the one choice that weighs neighbours)


def smooth_stage(imgs, dev):
    taps = U.gauss_taps(1.5)[1]
    params = capi.make_params(tol=0.0)
    with torch_io.Segmenter(N, H, W, 1, params=params, options=OPTIONS, smooth=(1.5, "blur")) as seg:
        masks, steps, norms = seg.segment(dev, STEPS)
        got_m, got_p = masks.cpu().numpy(), seg.images().cpu().numpy()
    for i in range(N):
        assert np.array_equal(got_p[i], U.blur(imgs[i], taps))
        with capi.Context(H, W, 1) as src, capi.Context(H, W, 1, params) as ctx:
            ctx.set_option("wave_pol", 0)
            src.set_image([imgs[i]])
            src.smooth_planes_to(ctx, 1.5, "blur")
            ctx.init_checkerboard()
            done, nrm = ctx.run(STEPS)
            assert done == steps[i]                                                  # (a context alone may take another data flow than
            assert np.array_equal(ctx.get_mask(), got_m[i])                          # a batch member: masks and counts, as torch_window_child.py)
    # rank -> smooth -> local: a median, the detail under a box, the local mean -- each stage sees what the one before has made
    box = list(U.box_taps(2))
    with torch_io.Segmenter(N, H, W, 1, options=OPTIONS, rank=(1, "median"), smooth=(box, (U.COPY, U.BLUR, U.DETAIL)), local=(2, "mean")) as seg:
        assert seg.run_channels == 3 and len(seg.ranked) == len(seg.smoothed) == N
        seg.segment(dev, 2)
        got = seg.images().cpu().numpy()
    for i in range(N):
        ranked = RU.expected([imgs[i]], 1, 1, (RU.MEDIAN, 0, 0))
        smoothed = U.expected(ranked, 3, box, (U.COPY, U.BLUR, U.DETAIL))
        assert np.array_equal(got[i], np.stack(LU.expected(smoothed, 3, 2, (LU.MEAN,) * 3)))


def edge_sigma(imgs, dev):
    taps = U.gauss_taps(2.0)[1]
    params = capi.make_params(tol=0.0, mu=5.0, lambda1=[1e-3] * 3, lambda2=[1e-3] * 3)
    with torch_io.Segmenter(N, H, W, 1, params=params, edge=K, edge_sigma=2) as seg:
        assert len(seg.edge_sources) == N
        masks, steps, norms = seg.segment(dev, STEPS, init="otsu")
        got_m, got_u, got_g, got_p = masks.cpu().numpy(), seg.levelsets().cpu().numpy(), seg.edge_maps().cpu().numpy(), seg.images().cpu().numpy()
    for i in range(N):
        assert np.array_equal(got_p[i], imgs[i])                                     # the run iterates on the unblurred planes
        assert np.array_equal(got_g[i], G.edge_map([U.blur(imgs[i], taps)], K))     # g of G_sigma * I
        assert not np.array_equal(got_g[i], G.edge_map([imgs[i]], K))
        with capi.Context(H, W, 1, params) as ctx, capi.Context(H, W, 1) as scratch:
            ctx.set_image([imgs[i]])
            ctx.init_otsu()
            ctx.smooth_planes_to(scratch, 2.0, "blur")
            ctx.edge_map_from(scratch, K)
            done, nrm, _ = capi.geodesic_run(ctx, STEPS)
            assert done == steps[i] == STEPS and nrm == norms[i]
            assert np.array_equal(ctx.get_edge_map(), got_g[i])
            assert np.array_equal(ctx.get_mask(), got_m[i])
            assert np.array_equal(ctx.get_levelset().view(np.uint64), got_u[i].view(np.uint64))


def main():
    imgs = np.stack([G.demo_scene()[0], np.ascontiguousarray(G.demo_scene()[0].T)])
    dev = torch.from_numpy(imgs).cuda()
    smooth_stage(imgs, dev)
    edge_sigma(imgs, dev)
    print("torch_smooth child ok")


if __name__ == "__main__":
    main()
