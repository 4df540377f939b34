"""Child process of test_gpu_torch_split.py: torch first, then the library -- one HIP runtime.  On device tensors of two shapes
(2 x 48 x 80 and 2 x 37 x 71): Segmenter.split equals the restatement (split_util.py) of the segmenter's own masks, one radius for all and
one per member, with and without cleaning; after Segmenter.split_levelset the level sets, components, measure, contours, overlaps and match
are those of F0 \\ cut; a bad radius is a ValueError.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import components_util as CU  # noqa: E402
import contour_util as CT  # noqa: E402
import split_util as S  # noqa: E402
from chan_vese_amd import capi, torch_io  # noqa: E402

N = 2


def main():
    params = capi.make_params(tol=0.0)
    for h, w in ((48, 80), (37, 71)):
        f0 = np.stack([S.CASES["touching"](h, w), S.CASES["noisy"](h, w)])
        with torch_io.Segmenter(N, h, w, 1, params=params) as seg:
            for i, c in enumerate(seg._phase(0)):                       # (measure reads the planes)
                c.set_image([np.random.default_rng(i).integers(0, 256, size=(h, w), dtype=np.uint8)])
            start = torch.from_numpy(f0.astype(np.uint8)).cuda()
            torch.cuda.synchronize()
            capi.init_mask_batch(seg._phase(0), [start[i].data_ptr() for i in range(N)])
            assert np.array_equal(seg.clean_masks().cpu().numpy() != 0, f0)
            for conn in (4, 8):
                for radius in (0.0, 2.0, [3.0, 1.5]):
                    labels, counts = seg.split(radius, conn=conn)
                    assert labels.dtype == torch.int32 and labels.is_cuda and tuple(labels.shape) == (N, h, w)
                    for i in range(N):
                        want = S.Split(f0[i], conn, capi.r2_of(radius[i] if isinstance(radius, list) else radius))
                        assert counts[i] == want.K and np.array_equal(labels[i].cpu().numpy(), want.labels), (conn, radius, i)
            labels, counts = seg.split(2.0, min_area=5, fill_holes=-1)
            for i in range(N):
                want = S.Split(CU.clean(f0[i], 4, 5, -1, False).astype(bool), 4, 4)
                assert counts[i] == want.K and np.array_equal(labels[i].cpu().numpy(), want.labels), i
            # in place: the other mask calls see the split objects
            seg.split_levelset(2.0)
            want = [S.Split(f0[i], 4, 4) for i in range(N)]
            assert np.array_equal(seg.levelsets().cpu().numpy(), np.stack([np.where(s.pieces, 1.0, -1.0) for s in want]))
            for conn in (4, 8):
                labels, counts = seg.components(conn=conn)
                for i in range(N):
                    lab, table = CU.label(want[i].pieces, conn)
                    assert counts[i] == table.size and np.array_equal(labels[i].cpu().numpy(), lab), (conn, i)
            for i in range(N):
                assert int(seg.measure()[i][1]["area"].sum()) == int(want[i].pieces.sum())
            # contours, overlaps and match see the split objects too: against the split's own labels every piece matches its object
            found = seg.contours(conn=4)
            truth = torch.from_numpy(np.stack([s.labels * s.pieces for s in want]).astype(np.int32)).cuda()
            rows, matches = seg.overlaps(truth), seg.match(truth)
            for i in range(N):
                lab, table = CU.label(want[i].pieces, 4)
                assert found[i][0].size == CT.trace(want[i].pieces, 4, True)[0].size, i
                pairs = rows[i][(rows[i]["a"] > 0) & (rows[i]["b"] > 0)]
                assert pairs.size == table.size and int(pairs["count"].sum()) == int(want[i].pieces.sum()), i   # a piece lies in ONE object
                score = matches[i][0]
                objects = np.unique(truth[i].cpu().numpy()).size - 1            # (the cut may leave an object in several pieces)
                assert score.tp + score.fp == table.size and score.tp + score.fn == objects and score.tp > 0, (i, score)
            for bad in (-1.0, float("nan"), [1.0]):
                try:
                    seg.split(bad)
                except ValueError:
                    continue
                raise AssertionError(f"no ValueError for {bad!r}")
    print("torch_split child ok")


if __name__ == "__main__":
    main()
