"""Child process of test_gpu_torch_local.py and test_gpu_torch_rank.py: torch first, then the library -- one HIP runtime.  The argument
names the family, "local" or "rank".  Segmenter(local=(R, what)) / Segmenter(rank=(R, what)) on 3 x 64 x 48 device tensors against the
capi sequence (set_image, local_planes_to / rank_planes_to, the start, run, get_mask) and against a Segmenter without the option fed the
restated planes (local_util, rank_util):
  local  the 1 -> 1 deviation, the 1 -> 3 stack, per-channel deviations of three planes, a 3 -> 1 mean; the local planes come behind
         Perona-Malik; levels=2 takes them in front of the restricts.
  rank   the 1 -> 1 median and top-hat, per-channel closings of three planes, a 3 -> 1 maximum, a 1 -> 3 triple; with local= as well the
         rank filter runs first and the local statistics are taken of its result; the rank planes come behind Perona-Malik.
Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, torch_io  # noqa: E402
import local_util as LU  # noqa: E402
import rank_util as RU  # noqa: E402

N, H, W, STEPS = 3, 64, 48, 30
OPTIONS = {"wave_pol": 0}   # (batch members never take the resident flow; the cache policy is the one choice that weighs neighbours)
PM = (30.0, 0.25, 1.0)
PARAMS = dict(lambda1=[0.5, 1, 1], lambda2=[0.5, 1, 1])


def run(images, channels, **kw):
    """one Segmenter's life: (masks, steps, norms, images(), level sets as bit patterns) on the host"""
    seg_kw = {k: kw.pop(k) for k in ("rank", "local", "levels") if k in kw}
    with torch_io.Segmenter(N, H, W, channels, params=capi.make_params(**PARAMS), options=OPTIONS, **seg_kw) as seg:
        masks, steps, norms = seg.segment(images, STEPS, **kw)
        return masks.cpu().numpy(), steps, norms, seg.images().cpu().numpy(), seg.levelsets().cpu().numpy().view(np.uint64)


def same(a, b, what):
    assert a[1] == b[1] and a[2] == b[2], (what, a[1:3], b[1:3])
    for x, y in zip((a[0], a[3], a[4]), (b[0], b[3], b[4])):
        assert np.array_equal(x, y), what


def capi_sequence(family, member, src_channels, run_channels, R, codes, init):
    """the masks of the sequence, one member at a time"""
    with capi.Context(H, W, src_channels) as src, capi.Context(H, W, run_channels, capi.make_params(**PARAMS)) as ctx:
        ctx.set_option("wave_pol", 0)
        src.set_image(list(member) if src_channels == 3 else [member])
        getattr(src, family + "_planes_to")(ctx, R, codes)
        ctx.init_otsu() if init == "otsu" else ctx.init_checkerboard()
        steps, _ = ctx.run(STEPS)
        return ctx.get_mask(), steps


def cases_equal_the_sequences(family, U, cases):
    for imgs, cs, cd, R, what, codes in cases:
        want = np.stack([np.stack(U.expected(list(m) if cs == 3 else [m], cd, R, codes)) for m in imgs])
        want = want[:, 0] if cd == 1 else want
        dev_in, dev_want = torch.from_numpy(imgs).cuda(), torch.from_numpy(want).cuda()
        for init in ("checkerboard", "otsu"):      # (Otsu sees the family's planes)
            got = run(dev_in, cs, init=init, **{family: (R, what)})
            assert np.array_equal(got[3], want), (what, init)
            same(got, run(dev_want, cd, init=init), (what, init, "restated planes"))
            for i in range(N):
                mask, steps = capi_sequence(family, imgs[i], cs, cd, R, codes, init)
                assert steps == got[1][i] and np.array_equal(mask, got[0][i]), (what, init, i)


def local(grey, rgb):
    U = LU
    cases_equal_the_sequences("local", U, [(grey, 1, 1, 2, "dev", (U.DEV,)), (grey, 1, 3, 3, "stack", U.STACK), (rgb, 3, 3, 1, "dev", (U.DEV,) * 3),
                                           (rgb, 3, 1, 4, (U.MEAN,), (U.MEAN,))])
    # the local planes come after the smoothing
    dev_in = torch.from_numpy(grey).cuda()
    smoothed = run(dev_in, 1, perona_malik=PM)[3]
    assert not np.array_equal(smoothed, grey)
    got = run(dev_in, 1, local=(2, "stack"), perona_malik=PM)
    assert np.array_equal(got[3], np.stack([np.stack(U.expected([m], 3, 2, U.STACK)) for m in smoothed]))
    same(got, run(torch.from_numpy(got[3]).cuda(), 3), "Perona-Malik")
    # levels = 2: the local planes on the finest level, in front of the restricts
    want = np.stack([U.expected([m], 1, 2, (U.DEV,))[0] for m in grey])
    same(run(dev_in, 1, local=(2, "dev"), levels=2, init="otsu"), run(torch.from_numpy(want).cuda(), 1, levels=2, init="otsu"), "levels")


def rank(grey, rgb):
    U = RU
    cases_equal_the_sequences("rank", U, [(grey, 1, 1, 2, "median", (U.MEDIAN,)), (grey, 1, 1, 9, "tophat", (U.TOPHAT,)), (rgb, 3, 3, 3, "close", (U.CLOSE,) * 3),
                                          (rgb, 3, 1, 4, (U.MAX,), (U.MAX,)), (grey, 1, 3, 2, (U.COPY, U.OPEN, U.TOPHAT), (U.COPY, U.OPEN, U.TOPHAT))])
    # with local= as well the rank filter runs first and the local statistics are taken of its result
    dev_in = torch.from_numpy(grey).cuda()
    got = run(dev_in, 1, rank=(1, "median"), local=(2, "stack"))
    want = np.stack([np.stack(LU.expected([U.fast(m, 1, U.MEDIAN)], 3, 2, LU.STACK)) for m in grey])
    assert np.array_equal(got[3], want)
    same(got, run(torch.from_numpy(want).cuda(), 3), "rank then local")
    # the rank planes come after the smoothing
    smoothed = run(dev_in, 1, perona_malik=PM)[3]
    assert not np.array_equal(smoothed, grey)
    got = run(dev_in, 1, rank=(3, "open"), perona_malik=PM)
    assert np.array_equal(got[3], np.stack([U.fast(m, 3, U.OPEN) for m in smoothed]))
    same(got, run(torch.from_numpy(got[3]).cuda(), 1), "Perona-Malik")


def main(family):
    U = {"local": LU, "rank": RU}[family]
    grey = np.stack([U.blocky_planes(H, W, 1, seed=30 + i)[0] for i in range(N)])                           # (N, H, W)
    rgb = np.stack([np.stack(U.blocky_planes(H, W, 3, seed=40 + i)) for i in range(N)])                     # (N, 3, H, W)
    {"local": local, "rank": rank}[family](grey, rgb)
    print(f"torch_{family} child ok")


if __name__ == "__main__":
    main(sys.argv[1])
