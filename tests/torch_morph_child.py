"""Child process of test_gpu_torch_morph.py: torch first, then the library -- one HIP runtime.  On device tensors of two shapes (two
segmenters: 2 x 48 x 80 and 2 x 33 x 257): clean_masks(morph=...) and Segmenter.morph equal the restatement (morph_util.py) of the
segmenter's own masks, and components / measure / contours / score afterwards see the morphed set; segment(init=("mask", t)), bool and
uint8, equals a Segmenter started from the same level sets; the levels > 1 refusal and the bad tensors are ValueErrors.  Exits non-zero on
the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_util as CU  # noqa: E402
import morph_util as M  # noqa: E402
from chan_vese_amd import capi, synth, torch_io  # noqa: E402

N, STEPS = 2, 24


def refused(call):
    try:
        call()
    except ValueError as e:
        return str(e)
    raise AssertionError("no ValueError")


def main():
    params = capi.make_params(tol=0.0)
    options = {"resident": 0, "co_resident": 0}
    for h, w in ((48, 80), (33, 257)):
        imgs = np.stack([synth.disk(64, 200, 50, noise=40 + 8 * i, seed=3 + i, h=h, w=w) for i in range(N)])
        dev = torch.from_numpy(imgs).cuda()
        with torch_io.Segmenter(N, h, w, 1, params=params, options=options) as seg:
            masks, steps, _ = seg.segment(dev, STEPS)
            assert steps == [STEPS] * N
            raw = masks.cpu().numpy() != 0
            # byte masks: every operation, one radius for all and one per member, with and without cleaning
            for op in ("dilate", "erode", "open", "close"):
                for radius in (1.0, 1.5, [2.3, 3.0]):
                    got = seg.clean_masks(morph=op, radius=radius).cpu().numpy()
                    for i in range(N):
                        r2 = capi.r2_of(radius[i] if isinstance(radius, list) else radius)
                        assert np.array_equal(got[i], M.morph(raw[i], capi.morph_code(op), r2)), (op, radius, i)
            assert torch.equal(seg.clean_masks(), masks) and torch.equal(seg.clean_masks(morph="none", radius=3.0), masks)
            cleaned = seg.clean_masks(min_area=4, fill_holes=-1).cpu().numpy()
            got = seg.clean_masks(min_area=4, fill_holes=-1, morph="open", radius=2.0, invert=False).cpu().numpy()
            for i in range(N):
                assert np.array_equal(cleaned[i], CU.clean(raw[i], 4, 4, -1, False))
                assert np.array_equal(got[i], M.morph(cleaned[i] != 0, M.OPEN, 4)), i
            # in place: the other mask calls see the morphed set
            seg.morph("open", 1.5)
            want = np.stack([M.morph(raw[i], M.OPEN, 2) for i in range(N)])
            assert np.array_equal(seg.clean_masks().cpu().numpy(), want.astype(np.uint8))
            assert np.array_equal(seg.levelsets().cpu().numpy(), np.where(want, 1.0, -1.0))
            labels, counts = seg.components()
            for i in range(N):
                lab, table = CU.label(want[i], 4)
                assert counts[i] == table.size and np.array_equal(labels[i].cpu().numpy(), lab), i
                assert seg.measure()[i][0] == table.size and int(seg.measure()[i][1]["area"].sum()) == int(want[i].sum())
            scores = seg.score(torch.from_numpy(want).cuda())
            assert all(s.fp == 0 and s.fn == 0 for s in scores)
            assert len(seg.contours()) == N
            # a mask start equals a start from the same level sets: masks, steps, norms and the level sets behind them
            start = torch.from_numpy(want).cuda()
            a = seg.segment(dev, STEPS, init=("mask", start))
            ua = seg.levelsets().cpu().numpy()
            b = seg.segment(dev, STEPS, init=("mask", (start.to(torch.uint8) * 200).contiguous()))
            assert torch.equal(a[0], b[0]) and a[1:] == b[1:]
            c = seg.segment(dev, STEPS, init=torch.from_numpy(np.where(want, 1.0, -1.0)).cuda())
            assert torch.equal(a[0], c[0]) and a[1:] == c[1:] and a[1] == [STEPS] * N, (a[1:], c[1:])
            assert np.array_equal(ua.view(np.uint64), seg.levelsets().cpu().numpy().view(np.uint64))
            for bad in (start[:, :, :-1], start.to(torch.float32), start.cpu(), want):
                refused(lambda: seg.segment(dev, STEPS, init=("mask", bad)))
            refused(lambda: seg.clean_masks(morph="thin", radius=1.0))
            refused(lambda: seg.morph("open", -1.0))
        with torch_io.Segmenter(N, 64, 96, 1, params=params, levels=2) as pyr:
            msg = refused(lambda: pyr.segment(torch.zeros((N, 64, 96), dtype=torch.uint8).cuda(), 4, init=("mask", torch.zeros((N, 64, 96), dtype=torch.uint8).cuda())))
            assert "levels = 1" in msg and "not resampled" in msg, msg
    print("torch_morph child ok")


if __name__ == "__main__":
    main()
