"""Child process of test_gpu_torch_measure.py: torch first, then the library -- one HIP runtime.  Segmenter.measure() after segment() on
device tensors (2 x 48 x 80 grey and 2 x 33 x 257 colour), on a side stream made current, equals Context.measure() of the segmenter's own
contexts and the restatement (measure_util.py) on the masks and planes the segmenter returns.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import measure_util as mu  # noqa: E402
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
                for args in ((4, False, 0, 0, False), (8, True, 0, 0, False), (4, False, 3, -1, True)):
                    got = seg.measure(*args)
                    clean = seg.clean_masks(*args)
                    side.synchronize()
                    host = clean.cpu().numpy()
                    for i, c in enumerate(seg.contexts):
                        k, t = c.measure(*args)
                        assert got[i][0] == k and got[i][1].tobytes() == t.tobytes(), (args, i)
                        want = mu.measure(host[i] != 0, list(planes[i]), args[0])
                        mu.assert_tables_equal(t, want, (args, i))
                        mu.assert_shapes_match(capi.region_shapes(t, channels), t, channels)
                capped = seg.measure(cap=2)
                assert all(t.size == min(k, 2) for k, t in capped)
    print("torch_measure child ok")


if __name__ == "__main__":
    main()
