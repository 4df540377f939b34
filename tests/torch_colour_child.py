"""Child process of test_gpu_torch_colour.py: torch first, then the library -- one HIP runtime.  Segmenter(colour="ycrcb", order="rgb") on
3 x 64 x 48 x 3 device tensors against a Segmenter with colour=None fed the restated planes (colour_util), for both layouts; the
conversion behind Perona-Malik; levels=2.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, torch_io  # noqa: E402
import colour_util as U  # noqa: E402

N, H, W, STEPS = 3, 64, 48, 30
OPTIONS = {"wave_pol": 0}   # (batch members never take the resident flow; the cache policy is the one choice that weighs neighbours)
PM = (30.0, 0.25, 1.0)


def run(images, layout=None, **kw):
    """one Segmenter's life: (masks, steps, norms, images(), level sets as bit patterns) on the host"""
    seg_kw = {k: kw.pop(k) for k in ("colour", "order", "levels") if k in kw}
    with torch_io.Segmenter(N, H, W, 3, params=capi.make_params(lambda1=[0.1, 1, 1], lambda2=[0.1, 1, 1]), options=OPTIONS, **seg_kw) as seg:
        masks, steps, norms = seg.segment(images, STEPS, layout=layout, **kw)
        return masks.cpu().numpy(), steps, norms, seg.images().cpu().numpy(), seg.levelsets().cpu().numpy().view(np.uint64)


def same(a, b, what):
    assert a[1] == b[1] and a[2] == b[2], (what, a[1:3], b[1:3])
    for x, y in zip((a[0], a[3], a[4]), (b[0], b[3], b[4])):
        assert np.array_equal(x, y), what


def main():
    rgb = np.stack([np.stack(U.planes_of("random", H, W, "rgb", seed=20 + i)) for i in range(N)])          # (N, 3, H, W)
    rgb[:, :, 16:48, 12:36] //= 2                                                                          # something to segment
    for space, order in (("ycrcb", "rgb"), ("yuv", "bgr")):
        want = np.stack([np.stack(U.forward(list(img), space, order)) for img in rgb])
        planar, planar_want = torch.from_numpy(rgb).cuda(), torch.from_numpy(want).cuda()
        inter = torch.from_numpy(np.ascontiguousarray(rgb.transpose(0, 2, 3, 1))).cuda()
        inter_want = torch.from_numpy(np.ascontiguousarray(want.transpose(0, 2, 3, 1))).cuda()
        for init in ("checkerboard", "otsu"):      # (Otsu sees the converted planes)
            ref = run(planar_want, init=init)
            assert np.array_equal(ref[3], want)
            same(run(planar, colour=space, order=order, init=init), ref, (space, order, init, "planar"))
            same(run(inter, capi.LAYOUT_INTERLEAVED, colour=space, order=order, init=init), ref, (space, order, init, "interleaved"))
            same(run(inter_want, capi.LAYOUT_INTERLEAVED, init=init), ref, (space, order, init, "interleaved, restated"))
        # the conversion comes after the smoothing: images() is forward(the Perona-Malik planes)
        smoothed = run(planar, perona_malik=PM)[3]
        assert not np.array_equal(smoothed, rgb)
        got = run(planar, colour=space, order=order, perona_malik=PM)
        assert np.array_equal(got[3], np.stack([np.stack(U.forward(list(img), space, order)) for img in smoothed])), (space, order)
        same(got, run(torch.from_numpy(got[3]).cuda()), (space, order, "Perona-Malik"))
        # levels = 2: the conversion on the finest level, in front of the restricts
        same(run(planar, colour=space, order=order, levels=2, init="otsu"), run(planar_want, levels=2, init="otsu"), (space, order, "levels"))
    print("torch_colour child ok")


if __name__ == "__main__":
    main()
