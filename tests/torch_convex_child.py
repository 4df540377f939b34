"""Child process of test_gpu_torch_convex.py: torch first, then the library -- one HIP runtime.  Segmenter(convex=...) on two 64 x 64
device tensors returns the masks, level sets and relaxed functions of the capi path (contexts fed the same inputs call for call:
init_checkerboard, edge_map_from, convex_run) byte for byte, plain and with edge=K; the plain run reaches the restatement's fixed point;
what does not compose is refused.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, torch_io  # noqa: E402
import convex_util as X  # noqa: E402

N, H, W, STEPS, K = 2, 64, 64, 12, 15.0


def main():
    img = X.disk_scene()[0]
    imgs = np.stack([img, np.ascontiguousarray(img.T)])
    dev = torch.from_numpy(imgs).cuda()
    params = capi.make_params(tol=0.0, mu=0.5, lambda1=[1e-3] * 3, lambda2=[1e-3] * 3)
    for edge, convex in ((None, 0.25), (K, (0.25, 0.5)), (None, dict(tau=0.5, stop_rms=-1.0, means_every=2))):
        with torch_io.Segmenter(N, H, W, 1, params=params, edge=edge, convex=convex) as seg:
            masks, steps, norms = seg.segment(dev, STEPS, init="checkerboard")
            assert masks.dtype == torch.uint8 and tuple(masks.shape) == (N, H, W) and np.isfinite(norms).all()
            v = seg.relaxed()
            assert v.dtype == torch.float64 and tuple(v.shape) == (N, H, W)
            got_m, got_u, got_v = masks.cpu().numpy(), seg.levelsets().cpu().numpy(), v.cpu().numpy()
            assert seg.components()[1] == [c.components(cap=0)[0] for c in seg.contexts]   # everything after the run is unchanged
            for bad in (dict(reinit_every=4), dict(energy_every=4)):
                try:
                    seg.segment(dev, STEPS, **bad)
                except ValueError:
                    continue
                raise AssertionError(bad)
        q = dict(torch_io.check_convex(convex), use_edge=edge is not None)
        for i in range(N):
            with capi.Context(H, W, 1, params) as ctx:
                ctx.set_image([imgs[i]])
                ctx.init_checkerboard()
                if edge is not None:
                    ctx.edge_map_from(ctx, K)
                done, nrm, _ = capi.convex_run(ctx, STEPS, q)
                assert done == steps[i] and nrm == norms[i]
                assert np.array_equal(ctx.get_mask(), got_m[i])
                assert np.array_equal(ctx.get_levelset().view(np.uint64), got_u[i].view(np.uint64))
                assert np.array_equal(ctx.relaxed().view(np.uint64), got_v[i].view(np.uint64))
        if edge is None and convex == 0.25:                                     # stop_rms = 0: the restatement's exact fixed point
            rv, rsteps, _ = X.disk_reference()
            assert abs(steps[0] - rsteps) <= 1 and norms[0] == 0.0 and np.array_equal(got_m[0], X.mask(rv - 0.5))
    with torch_io.Segmenter(N, H, W, 1, params=params) as seg:                     # the default takes none of the new branches
        assert seg.convex is None
        try:
            seg.relaxed()
        except ValueError:
            pass
        else:
            raise AssertionError("relaxed without convex=")
    for bad in (dict(convex=0), dict(convex=-1.0), dict(convex=float("nan")), dict(convex=float("inf")), dict(convex=True), dict(convex="0.25"),
                dict(convex=(0.5, 0.5)), dict(convex=dict(tau=0.25, rho=1)), dict(convex=0.25, phases=4), dict(convex=0.25, levels=2),
                dict(convex=0.25, localized=3)):
        try:
            torch_io.Segmenter(N, H, W, 1, **bad)
        except ValueError:
            continue
        raise AssertionError(bad)
    print("torch_convex child ok")


if __name__ == "__main__":
    main()
