"""Child process of test_gpu_torch_score.py: torch first, then the library -- one HIP runtime.  Segmenter.score() after segment() on device
tensors of two shapes (two segmenters: 2 x 48 x 80 and 2 x 33 x 257) equals Context.score() of the segmenter's own contexts on the same
data, host form and device form, and the restatement (score_util.py); bool and uint8 truth tensors agree.  Exits non-zero on the first
mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_util as S  # noqa: E402
from chan_vese_amd import capi, synth, torch_io  # noqa: E402

N, STEPS = 2, 24


def main():
    params = capi.make_params(tol=0.0)
    for h, w in ((48, 80), (33, 257)):
        imgs = np.stack([synth.disk(64, 200, 50, noise=8 + 4 * i, seed=3 + i, h=h, w=w) for i in range(N)])
        truth = np.stack([S.disk(h, w, h // 2 + i, w // 2 - 2 * i, min(h, w) // 4) for i in range(N)])
        dev = torch.from_numpy(imgs).cuda()
        t_bool = torch.from_numpy(truth).cuda()
        t_u8 = (t_bool.to(torch.uint8) * 255).contiguous()
        with torch_io.Segmenter(N, h, w, 1, params=params) as seg:
            masks, steps, _ = seg.segment(dev, STEPS)
            assert steps == [STEPS] * N
            got = seg.score(t_bool, tol=1.5)
            assert got == seg.score(t_u8, tol=1.5), (got, seg.score(t_u8, tol=1.5))
            host_masks = masks.cpu().numpy()
            for i, c in enumerate(seg.contexts):
                assert got[i] == c.score(truth[i], tol=1.5) == c.score(t_u8[i].data_ptr(), tol=1.5), (i, got[i])
                want = S.score(host_masks[i] != 0, truth[i], capi.score_tol2(1.5))
                assert S.as_dict(got[i]) == want, (i, S.as_dict(got[i]), want)
                assert got[i].iou == want["tp"] / (want["tp"] + want["fp"] + want["fn"]) and got[i].defined == 1
            inv = seg.score(t_bool, invert=True)
            assert [s.tp + s.fp for s in inv] == [h * w - (s.tp + s.fp) for s in got]
            for bad in (t_bool[:, :, :-1], t_bool.to(torch.float32), t_bool.cpu(), truth):
                try:
                    seg.score(bad)
                except ValueError:
                    continue
                raise AssertionError(type(bad))
    print("torch_score child ok")


if __name__ == "__main__":
    main()
