"""Child process of test_gpu_torch_init.py: torch first, then the library -- one HIP runtime.  Segmenter.segment with every device-side
start on 4 x 64 x 144 against the capi sequence, member by member.  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from chan_vese_amd import capi, synth, torch_io  # noqa: E402
import init_util as U  # noqa: E402

N, H, W, STEPS = 4, 64, 144, 12


def main():
    imgs = np.stack([synth.disk(H, 200 - 20 * i, 40 + 15 * i, noise=12, seed=30 + i, h=H, w=W) for i in range(N)])
    want_t = [U.otsu(U.histogram([imgs[i]])) for i in range(N)]
    forms = [
        ("otsu", lambda c, i: c.init_otsu()),
        (("threshold", 120), lambda c, i: c.init_threshold(120)),
        (("threshold", [90, 100, 110, 255]), lambda c, i: c.init_threshold([90, 100, 110, 255][i])),
        (("rect", (30, 10, 80, 40)), lambda c, i: c.init_rect(30, 10, 80, 40)),
        (("rect", [(0, 0, 10, 10), (-5, 20, 60, 90), (100, 5, 44, 50), (40, 40, 1, 1)]),
         lambda c, i: c.init_rect(*[(0, 0, 10, 10), (-5, 20, 60, 90), (100, 5, 44, 50), (40, 40, 1, 1)][i])),
        (("disk", (72, 32, 25)), lambda c, i: c.init_disk(72, 32, 25)),
        (("disk", [(72, 32, 0), (0, 0, 50), (200, 32, 70), (72, 32, 300)]),
         lambda c, i: c.init_disk(*[(72, 32, 0), (0, 0, 50), (200, 32, 70), (72, 32, 300)][i])),
    ]
    # level sets are compared in bits between two populations of contexts, so neither may see the other (tests/torch_io_child.py)
    host = [capi.Context(H, W, 1) for _ in range(N)]
    for ctx in host:
        ctx.set_option("co_resident", 0)
    t = torch.from_numpy(imgs).cuda()
    with torch_io.Segmenter(N, H, W, 1, options={"co_resident": 0}) as seg:
        assert seg.thresholds is None
        for init, own in forms:
            for pm in (None, (30.0, 0.25, 1.0)):
                if pm and init != "otsu":
                    continue
                for i, ctx in enumerate(host):
                    ctx.set_image([imgs[i]])
                if pm:
                    capi.perona_malik_batch(host, *pm)
                got_t = [own(ctx, i) for i, ctx in enumerate(host)]
                starts = [ctx.get_levelset() for ctx in host]
                res = capi.run_batch(host, STEPS)
                masks, steps, norms = seg.segment(t, STEPS, perona_malik=pm, init=init)
                assert list(zip(steps, norms)) == res, init
                for i, ctx in enumerate(host):
                    assert np.array_equal(masks[i].cpu().numpy(), ctx.get_mask()), (init, i)
                    assert np.array_equal(seg.levelsets()[i].cpu().numpy().view(np.uint64), ctx.get_levelset().view(np.uint64)), (init, i)
                if init == "otsu":
                    assert seg.thresholds == got_t, (seg.thresholds, got_t)
                    if not pm:
                        assert seg.thresholds == want_t
                        assert all(np.array_equal(starts[i], U.start_threshold([imgs[i]], want_t[i], 1.0, -1.0)) for i in range(N))
        for bad in (("rect", (1, 2, 3)), "sobel", ("threshold", 256)):
            try:
                seg.segment(t, STEPS, init=bad)
            except ValueError:
                continue
            raise AssertionError(f"a malformed init {bad!r} was accepted")
    for ctx in host:
        ctx.close()
    print("torch_init child ok")


if __name__ == "__main__":
    main()
