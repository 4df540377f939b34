"""Child process of test_gpu_torch_contour.py: torch first, then the library -- one HIP runtime.  Segmenter.contours() after segment() on
device tensors (2 x 48 x 80 grey and 2 x 33 x 257 colour), on a side stream made current, equals Context.contours() of the segmenter's own
contexts and the restatement (contour_util.py) on the masks the segmenter returns.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contour_util as ct  # noqa: E402
from chan_vese_amd import capi, synth, torch_io  # noqa: E402

N, STEPS = 2, 24


def main():
    params = capi.make_params(tol=0.0)
    side = torch.cuda.Stream()
    for h, w, channels in ((48, 80, 1), (33, 257, 3)):
        planes = np.stack([np.stack([synth.disk(64, 200 - 25 * k, 50 + 15 * k, noise=24 + 4 * i, seed=3 + i + 7 * k, h=h, w=w) for k in range(channels)])
                           for i in range(N)])
        dev = torch.from_numpy(planes[:, 0] if channels == 1 else planes).cuda()
        with torch_io.Segmenter(N, h, w, channels, params=params) as seg:
            with torch.cuda.stream(side):
                masks, steps, _ = seg.segment(dev, STEPS)
                assert steps == [STEPS] * N
                for args in ((8, False, 0, 0, False, True), (4, True, 0, 0, False, False), (4, False, 3, -1, True, True)):
                    got = seg.contours(*args)
                    clean = seg.clean_masks(*args[:5])
                    side.synchronize()
                    host = clean.cpu().numpy()
                    for i, c in enumerate(seg.contexts):
                        loops, points = got[i]
                        assert points.dtype == torch.int32 and points.is_cuda and points.shape == (int(loops["points"].sum()), 2)
                        alone = c.contours(*args)
                        assert loops.tobytes() == alone[0].tobytes() and np.array_equal(points.cpu().numpy(), alone[1]), (args, i)
                        ct.assert_equal(alone, ct.trace(host[i] != 0, args[0], args[5]), (args, i))
                        assert loops.size >= 1
    print("torch_contour child ok")


if __name__ == "__main__":
    main()
