"""Child process of test_gpu_components.py: torch first, then the library -- one HIP runtime (tests/torch_io_child.py's pattern).
Segmenter.components and Segmenter.clean_masks on a caller stream against the numpy restatement.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from chan_vese_amd import synth, torch_io  # noqa: E402
import components_util as cu  # noqa: E402

N, H, W, STEPS = 5, 100, 176, 10


def main():
    imgs = np.stack([synth.disk(max(H, W), 200 - 9 * i, 50 + 7 * i, noise=32, seed=40 + i, h=H, w=W) for i in range(N)])
    with torch_io.Segmenter(N, H, W, 1, options={"co_resident": 0}) as seg:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            t = torch.from_numpy(imgs).cuda()
            seg.segment(t, STEPS)
            u = seg.levelsets().cpu().numpy()
            for conn, invert in ((4, False), (8, True)):
                labels, counts = seg.components(conn, invert)
                top = labels.amax(dim=(1, 2))                      # enqueued right behind the call on the side stream
                clean = seg.clean_masks(conn, invert, 5, -1, True)
                area = clean.sum(dim=(1, 2))
                assert labels.dtype == torch.int32 and tuple(labels.shape) == (N, H, W) and labels.is_cuda
                assert clean.dtype == torch.uint8 and tuple(clean.shape) == (N, H, W) and clean.is_cuda
                top, area = top.cpu().numpy(), area.cpu().numpy()
                for i in range(N):
                    f = cu.foreground(u[i], invert)
                    want_l, want_t = cu.label(f, conn)
                    want_c = cu.clean(f, conn, 5, -1, True)
                    assert counts[i] == want_t.size == top[i], (conn, invert, i)
                    assert np.array_equal(labels[i].cpu().numpy(), want_l), (conn, invert, i)
                    assert np.array_equal(clean[i].cpu().numpy(), want_c) and area[i] == want_c.sum(), (conn, invert, i)
            plain = seg.clean_masks()
            assert np.array_equal(plain.cpu().numpy(), cu.foreground(u).astype(np.uint8))
        side.synchronize()
    print("torch components child ok")


if __name__ == "__main__":
    main()
