"""Child process of test_gpu_torch_overlap.py: torch first, then the library -- one HIP runtime.  Segmenter.overlaps() / .match() on three
members of mixed content against a grid of squares on the device equal Context.overlaps() of the segmenter's contexts, the restatement
(overlap_util.py) and its brute-force match; and frame to frame: the tensors components() returned for frame 1 are the labels for frame 2,
a disk shifted by 3 pixels, where every object matches at 1/2.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_util as cu  # noqa: E402
import overlap_util as ou  # noqa: E402
from chan_vese_amd import capi, torch_io  # noqa: E402

N, H, W = 3, 48, 80


def disks(centres, r, h=H, w=W):
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for cy, cx in centres:
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m


def set_masks(seg, masks):
    for c, m in zip(seg.contexts, masks):
        c.set_levelset(np.where(m, 1.0, -1.0))


def main():
    rng = np.random.default_rng(11)
    side = torch.cuda.Stream()
    images = torch.from_numpy(rng.integers(0, 256, (N, H, W), dtype=np.uint8)).cuda()
    with torch_io.Segmenter(N, H, W, 1, params=capi.make_params(tol=0.0)) as seg:
        for c, img in zip(seg.contexts, images.cpu().numpy()):
            c.set_image([img])
        # mixed content: noise, three disks, nothing
        masks = [rng.random((H, W)) < 0.5, disks([(12, 14), (30, 40), (20, 66)], 8), np.zeros((H, W), bool)]
        set_masks(seg, masks)
        truth = np.stack([ou.grid_labels(H, W, 16), (np.where(disks([(13, 15)], 8), 5, 0) + np.where(disks([(30, 41)], 8), 6, 0) +
                           np.where(disks([(40, 8)], 4), 9, 0)).astype(np.int32), ou.grid_labels(H, W, 16) - 3])
        with torch.cuda.stream(side):
            labels = torch.from_numpy(truth).cuda()
            for args in ((4, False, 0, 0, False), (8, True, 0, 0, False), (4, False, 3, -1, True)):
                got = seg.overlaps(labels, *args)
                as_list = seg.overlaps([labels[i] for i in range(N)], *args)
                matched = seg.match(labels, 0.5, *args)
                for i, c in enumerate(seg.contexts):
                    own, _ = c.overlaps(truth[i], *args)
                    want, _ = ou.overlaps(masks[i] != args[1], truth[i], args[0], args[2], args[3], args[4])
                    ou.assert_rows_equal(got[i], want, (args, i))
                    assert own.tobytes() == got[i].tobytes() == as_list[i].tobytes()
                    score, match_of_a, ious = matched[i]
                    brute = ou.match(want, 1, 2)
                    assert (score.objects_a, score.objects_b, score.tp, score.fp, score.fn) == brute[:5] and match_of_a.tolist() == brute[5]
                    assert score.tp_at == tuple(ou.match(want, q, 20)[2] for q in range(10, 20)) and len(ious) == score.tp
            s = seg.match(labels, (1, 2))[1][0]
            assert (s.objects_a, s.objects_b, s.tp, s.fp, s.fn) == (3, 3, 2, 1, 1) and s.precision == 2 / 3 and s.recall == 2 / 3
            for bad in (labels.to(torch.int64), labels[:2], labels.cpu(), labels[:, :, :-1]):
                try:
                    seg.overlaps(bad)
                except ValueError:
                    continue
                raise AssertionError("a wrong labels tensor was accepted")
            # frame to frame: the disks move by 3 pixels; the labels of frame 1 stay on the device
            centres = [(12, 14), (30, 40), (20, 66)]
            set_masks(seg, [disks(centres[:k + 1], 8) for k in range(N)])
            frame1, counts1 = seg.components()
            set_masks(seg, [disks([(cy + 3, cx) for cy, cx in centres[:k + 1]], 8) for k in range(N)])
            res = seg.match(frame1)
            side.synchronize()
            for k, (score, match_of_a, ious) in enumerate(res):
                assert counts1[k] == k + 1 and (score.objects_a, score.objects_b, score.tp, score.fp, score.fn) == (k + 1, k + 1, k + 1, 0, 0)
                assert match_of_a.tolist() == list(range(1, k + 2)) and score.mean_ap > 0.2
                host1, _ = cu.label(disks(centres[:k + 1], 8), 4)
                assert np.array_equal(frame1[k].cpu().numpy(), host1)
    print("torch_overlap child ok")


if __name__ == "__main__":
    main()
