"""Child process of test_gpu_torch_io.py: torch first, then the library -- one HIP runtime.  argv[1] is the form of the image tensor:
gray (N, H, W), planar3 (N, 3, H, W) or inter3 (N, H, W, 3).  Exits non-zero on the first mismatch."""
import os
import sys

import torch  # noqa: E402  (before chan_vese_amd: capi.py's rule)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from chan_vese_amd import capi, synth, torch_io  # noqa: E402

N, H, W, STEPS = 16, 128, 160, 40


def host_pipeline(ctxs, imgs, pm, init):
    """the host-buffer calls; imgs[i] is (C, H, W)"""
    for ctx, img in zip(ctxs, imgs):
        ctx.set_image(list(img))
    if pm:
        capi.perona_malik_batch(ctxs, *pm)
    for i, ctx in enumerate(ctxs):
        if init is None:
            ctx.init_checkerboard()
        else:
            ctx.set_levelset(init[i].astype(np.float64))
    res = capi.run_batch(ctxs, STEPS)
    return np.stack([ctx.get_mask() for ctx in ctxs]), res


def main(form):
    C = 1 if form == "gray" else 3
    imgs = np.stack([np.stack([synth.disk(H, 200 - 4 * i - 20 * k, 40 + 3 * i + 10 * k, noise=8, seed=100 * k + i, h=H, w=W) for k in range(C)])
                     for i in range(N)])                                   # (N, C, H, W)
    as_form = {"gray": lambda a: a[:, 0], "planar3": lambda a: a, "inter3": lambda a: a.transpose(0, 2, 3, 1)}[form]
    rng = np.random.default_rng(3)
    u0 = rng.standard_normal((N, H, W)) * 2.0
    # level sets are compared in bits between two populations of contexts, so neither may see the other: a context's automatic choices
    # (strip lengths) look at what else lives on the device (tests/test_gpu_device_io.py, same_choices)
    host = [capi.Context(H, W, C) for _ in range(N)]
    for ctx in host:
        ctx.set_option("co_resident", 0)
    with torch_io.Segmenter(N, H, W, C, options={"co_resident": 0}) as seg:
        for pm in (None, (30.0, 0.25, 2.0)):
            for init in (None, u0, u0.astype(np.float32)):
                if pm and init is not None and init.dtype == np.float32:
                    continue
                want, res = host_pipeline(host, imgs, pm, init)
                t = torch.from_numpy(np.ascontiguousarray(as_form(imgs))).cuda()
                ti = "checkerboard" if init is None else torch.from_numpy(init).cuda()
                masks, steps, norms = seg.segment(t, STEPS, perona_malik=pm, init=ti)
                total = masks.sum()                                      # enqueued right behind segment on the current stream: no host wait
                assert masks.dtype == torch.uint8 and tuple(masks.shape) == (N, H, W) and masks.is_cuda
                assert int(total.item()) == int(want.sum()), (form, pm, None if init is None else init.dtype)
                assert np.array_equal(masks.cpu().numpy(), want)
                assert list(zip(steps, norms)) == res
                inv, _, _ = seg.segment(t, STEPS, perona_malik=pm, init=ti, invert=True)
                assert np.array_equal(inv.cpu().numpy(), 1 - want)
                for i in (0, N - 1):
                    assert np.array_equal(seg.levelsets()[i].cpu().numpy(), host[i].get_levelset())
                    assert np.array_equal(seg.levelsets(torch.float32)[i].cpu().numpy(), host[i].get_levelset().astype(np.float32))
                    got = seg.images()[i].cpu().numpy().reshape(C, H, W)
                    assert np.array_equal(got, np.stack(host[i].get_image()))
        # the source written on a side stream made current, busy when segment is called: read complete, masks valid on that stream
        want, _ = host_pipeline(host, imgs, None, None)
        pinned = torch.from_numpy(np.ascontiguousarray(as_form(imgs))).pin_memory()
        side = torch.cuda.Stream()
        a = torch.zeros(128 << 20, dtype=torch.uint8, device="cuda")
        b = torch.empty_like(a)
        t = torch.zeros(pinned.shape, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(4):
                b.copy_(a, non_blocking=True)
            t.copy_(pinned, non_blocking=True)
            masks, _, _ = seg.segment(t, STEPS)
            total = masks.sum()
            got_total = int(total.item())     # read on the side stream: the default stream does not wait for a side stream
        assert got_total == int(want.sum())
        side.synchronize()
        assert np.array_equal(masks.cpu().numpy(), want)
        # a wrong tensor is refused before any library call
        for bad in (t.to(torch.float32), t[..., ::2] if form != "inter3" else t[:, :, ::2], t.cpu()):
            try:
                seg.segment(bad)
            except ValueError:
                continue
            raise AssertionError("a malformed tensor was accepted")
    for ctx in host:
        ctx.close()
    print("torch_io child ok:", form)


if __name__ == "__main__":
    main(sys.argv[1])
