"""Child process of test_gpu_torch_geodesic.py: torch first, then the library -- one HIP runtime.  Segmenter(edge=K) on two 64 x 64
device tensors, with a Perona-Malik stage in front, returns the masks, level sets and edge planes of the capi path (contexts fed the same
inputs call for call: perona_malik, edge_map_from, geodesic_run) byte for byte, and the edge planes equal the numpy restatement of the
smoothed planes; what does not compose is refused.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, torch_io  # noqa: E402
import geodesic_util as G  # noqa: E402

N, H, W, STEPS, K = 2, 64, 64, 12, 15.0
PM = (30.0, 0.25, 2.0)


def main():
    imgs = np.stack([G.demo_scene()[0], np.ascontiguousarray(G.demo_scene()[0].T)])
    dev = torch.from_numpy(imgs).cuda()
    params = capi.make_params(tol=0.0, mu=5.0, lambda1=[1e-3] * 3, lambda2=[1e-3] * 3)
    with torch_io.Segmenter(N, H, W, 1, params=params, edge=K) as seg:
        assert seg.edge == K
        masks, steps, norms = seg.segment(dev, STEPS, perona_malik=PM, init="otsu")
        assert masks.dtype == torch.uint8 and tuple(masks.shape) == (N, H, W) and steps == [STEPS] * N and np.isfinite(norms).all()
        maps = seg.edge_maps()
        assert maps.dtype == torch.uint16 and tuple(maps.shape) == (N, H, W)
        got_m, got_u, got_g = masks.cpu().numpy(), seg.levelsets().cpu().numpy(), maps.cpu().numpy()
        smoothed = seg.images().cpu().numpy()
        assert seg.components()[1] == [c.components(cap=0)[0] for c in seg.contexts]   # everything after the run is unchanged
        for bad in (dict(reinit_every=4), dict(energy_every=4)):
            try:
                seg.segment(dev, STEPS, **bad)
            except ValueError:
                continue
            raise AssertionError(bad)
    for i in range(N):
        assert np.array_equal(got_g[i], G.edge_map([smoothed[i]], K))             # built after the Perona-Malik stage
        with capi.Context(H, W, 1, params) as ctx:
            ctx.set_image([imgs[i]])
            ctx.perona_malik(*PM)
            ctx.init_otsu()
            ctx.edge_map_from(ctx, K)
            done, nrm, _ = capi.geodesic_run(ctx, STEPS)
            assert done == STEPS and nrm == norms[i]
            assert np.array_equal(ctx.get_edge_map(), got_g[i])
            assert np.array_equal(ctx.get_mask(), got_m[i])
            assert np.array_equal(ctx.get_levelset().view(np.uint64), got_u[i].view(np.uint64))
    with torch_io.Segmenter(N, H, W, 1, params=params) as seg:                     # the default takes none of the new branches
        assert seg.edge is None
        try:
            seg.edge_maps()
        except ValueError:
            pass
        else:
            raise AssertionError("edge_maps without edge=")
    for bad in (dict(edge=0), dict(edge=-1.0), dict(edge=float("nan")), dict(edge=float("inf")), dict(edge=True), dict(edge="30"),
                dict(edge=30.0, phases=4), dict(edge=30.0, levels=2), dict(edge=30.0, localized=3)):
        try:
            torch_io.Segmenter(N, H, W, 1, **bad)
        except ValueError:
            continue
        raise AssertionError(bad)
    print("torch_geodesic child ok")


if __name__ == "__main__":
    main()
