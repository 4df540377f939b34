"""Child process of test_gpu_torch_subpixel.py: torch first, then the library -- one HIP runtime.  Segmenter.contours(subpixel=True) after
segment() on device tensors (2 x 48 x 80 grey and 2 x 33 x 257 colour), on a side stream made current, equals Context.contours_subpixel()
of the segmenter's own contexts and the restatement (subpixel_util.py) on the level sets the segmenter holds; the default contours() is
the integer call it was.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contour_util as ct  # noqa: E402
import subpixel_util as su  # noqa: E402
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
                for args in ((8, False, 0, 0, False), (4, True, 0, 0, False), (4, False, 3, -1, True)):
                    got = seg.contours(*args, subpixel=True)
                    us = seg.levelsets()
                    side.synchronize()
                    host = us.cpu().numpy()
                    fractional = 0
                    for i, c in enumerate(seg.contexts):
                        loops, points = got[i]
                        assert points.dtype == torch.float64 and points.is_cuda and points.shape == (int(loops["edges"].sum()), 2)
                        alone = c.contours_subpixel(*args)
                        mine = points.cpu().numpy()
                        assert loops.tobytes() == alone[0].tobytes() and mine.tobytes() == alone[1].tobytes(), (args, i)
                        want = su.trace_subpixel(host[i], *args)
                        assert loops.tobytes() == want[0].tobytes() and mine.tobytes() == want[1].tobytes(), (args, i)
                        assert loops.size >= 1
                        fractional += int(np.count_nonzero(mine * 2 != np.round(mine * 2)))
                    print(f"{h} x {w} x {channels} {args}: {fractional} coordinates off the half-pixel grid, |u| in "
                          f"[{np.abs(host).min():.3g}, {np.abs(host).max():.3g}], {np.unique(host).size} distinct values")
                    assert fractional > 0 or any(args[2:])   # (an evolved level set: not every point of the raw mask's loops a midpoint)
                # the default call is the integer one, unchanged; simplify and subpixel do not go together
                for kwargs in ({}, {"simplify": False}, {"simplify": True, "conn": 4}):
                    got = seg.contours(**kwargs)
                    side.synchronize()
                    for i, c in enumerate(seg.contexts):
                        alone = c.contours(**kwargs)
                        assert got[i][1].dtype == torch.int32 and got[i][0].tobytes() == alone[0].tobytes()
                        assert np.array_equal(got[i][1].cpu().numpy(), alone[1])
                        ct.assert_equal(alone, ct.trace(c.get_mask() != 0, kwargs.get("conn", 8), kwargs.get("simplify", True)), (kwargs, i))
                for simplify in (True, False, 0):
                    try:
                        seg.contours(simplify=simplify, subpixel=True)
                    except ValueError as e:
                        assert "subpixel" in str(e)
                    else:
                        raise AssertionError(f"simplify={simplify!r} with subpixel=True was accepted")
    print("torch_subpixel child ok")


if __name__ == "__main__":
    main()
