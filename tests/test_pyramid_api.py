"""Coarse-to-fine without a GPU: the numpy restatement's own identities (pyramid_util), the exported symbols, capi.pyramid_shapes, the
Segmenter's and the CLI's validation of `levels` -- and the proposition itself on the CPU oracle: a 3-level pyramid over
synth.disk(256, noise=32, seed=3) needs fewer finest-level iterations than the one-level run and ends in the same mask."""
import os
import subprocess

import numpy as np
import pytest

import pyramid_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvh_restrict_image", "cvh_restrict_image_batch", "cvh_prolong_levelset", "cvh_prolong_levelset_batch"]


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    return m


@pytest.mark.parametrize("channels", U.CHANNELS)
@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_identities(shape, channels):
    h, w = shape
    hc, wc = U.coarse_shape(h, w)
    for kind in ("all255", "all0"):                       # no overflow, rounding at the top
        for q in U.planes_of(kind, h, w, channels):
            r = U.restrict(q)
            assert r.shape == (hc, wc) and r.dtype == np.uint8 and (r == q[0, 0]).all()
    small = U.planes_of("random", hc, wc, channels)
    for q in small:                                       # a 2 x 2-constant plane restricts to itself
        assert np.array_equal(U.restrict(U.prolong_mask(q, h, w)), q)
    for q in U.planes_of("random", h, w, channels):       # the definition, pixel by pixel, with the odd edge counted twice
        r = U.restrict(q)
        f = q.astype(int)
        for (rr, cc) in ((0, 0), (hc - 1, wc - 1), (hc - 1, 0), (0, wc - 1), (hc // 2, wc // 2)):
            r1, c1 = min(2 * rr + 1, h - 1), min(2 * cc + 1, w - 1)
            assert r[rr, cc] == (f[2 * rr, 2 * cc] + f[2 * rr, c1] + f[r1, 2 * cc] + f[r1, c1] + 2) >> 2
        if h % 2:
            assert np.array_equal(r[-1], U.restrict(np.vstack([q, q[-1:]]))[-1])
        if w % 2:
            assert np.array_equal(r[:, -1], ((f[0::2, -1] + f[np.minimum(np.arange(hc) * 2 + 1, h - 1), -1]) * 2 + 2) >> 2)
    u = U.special_levelset(hc, wc)
    up = U.prolong(u, h, w)
    assert up.shape == (h, w) and np.array_equal(U.bits(up)[::2, ::2], U.bits(u))
    assert np.array_equal(U.bits(up)[np.arange(h), :][:, np.arange(w)], U.bits(u)[np.arange(h) // 2][:, np.arange(w) // 2])
    assert set(U.SPECIALS.tolist()) <= set(U.bits(u).ravel().tolist())


def test_new_symbols_are_exported(capi):
    header = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name) and f"int {name}(" in header
    for name in ("restrict_image_batch", "prolong_levelset_batch", "run_coarse_to_fine", "run_coarse_to_fine_batch", "pyramid_shapes"):
        assert callable(getattr(capi, name))
    assert callable(capi.Context.restrict_image_to) and callable(capi.Context.prolong_levelset_to)
    assert "nothing is rescaled" in capi.run_coarse_to_fine.__doc__
    assert "Coarse-to-fine" in header and '"co_resident"' in header


def test_argument_errors_without_a_device(capi):
    L = capi.lib()
    assert L.cvh_restrict_image_batch(None, None, 1) == 1 and "cvh_restrict_image_batch" in L.cvh_last_error(None).decode()
    assert L.cvh_prolong_levelset_batch(None, None, 0) == 1
    assert L.cvh_restrict_image(None, None) == 1 and "pair 0" in L.cvh_last_error(None).decode()
    assert L.cvh_prolong_levelset(None, None) == 1
    with pytest.raises(ValueError):
        capi.restrict_image_batch([], [None])


def test_pyramid_shapes(capi):
    assert capi.pyramid_shapes(256, 256, 3) == [(256, 256), (128, 128), (64, 64)]
    assert capi.pyramid_shapes(33, 257, 2) == [(33, 257), (17, 129)]
    assert capi.pyramid_shapes(31, 50, 1) == [(31, 50)]
    assert capi.pyramid_shapes(64, 31, 2) == [(64, 31), (32, 16)]
    for h, w in U.SHAPES:
        for levels in (1, 2, 3):
            try:
                want = U.shapes(h, w, levels)
            except ValueError:
                with pytest.raises(ValueError):
                    capi.pyramid_shapes(h, w, levels)
            else:
                assert capi.pyramid_shapes(h, w, levels) == want
    for bad in ((64, 64, 0), (64, 64, -1), (64, 30, 2), (16, 16, 2), (15, 64, 1), (256, 256, 6)):
        with pytest.raises(ValueError):
            capi.pyramid_shapes(*bad)


def test_segmenter_validates_levels_without_a_gpu(capi):
    torch = pytest.importorskip("torch")
    from chan_vese_amd import torch_io
    assert torch_io.check_levels(3, 64, 144) == [(64, 144), (32, 72), (16, 36)]
    for bad in (0, -2, 4, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="levels|coarsest"):
            torch_io.check_levels(bad, 64, 144)
        with pytest.raises(ValueError):
            torch_io.Segmenter(2, 64, 144, levels=bad)           # refused before any context is created
    # the numbers of rect and disk are given in finest pixels: shifted right by levels - 1
    kind, rows = torch_io.check_init(("rect", (30, 10, 80, 40)), 2)
    assert torch_io.scale_init(kind, rows, 3) == [(7, 2, 20, 10)] * 2 and torch_io.scale_init(kind, rows, 1) == rows
    kind, rows = torch_io.check_init(("disk", [(72, 33, 25), (-5, 3, 7)]), 2)
    assert torch_io.scale_init(kind, rows, 2) == [(36, 16, 12), (-3, 1, 3)]
    assert torch_io.scale_init("threshold", [9, 9], 3) == [9, 9] and torch_io.scale_init("otsu", None, 3) is None
    seg = object.__new__(torch_io.Segmenter)
    seg.n, seg.h, seg.w, seg.channels, seg.device, seg.contexts, seg.thresholds, seg.levels = 2, 64, 144, 1, 0, [], None, 3
    images = torch.zeros((2, 64, 144), dtype=torch.uint8)
    with pytest.raises(ValueError, match="tensor init needs levels = 1"):
        seg.segment(images, init=torch.zeros((2, 64, 144), dtype=torch.float64))
    with pytest.raises(ValueError, match="reinit_every needs levels = 1"):
        seg.segment(images, reinit_every=5)
    with pytest.raises(ValueError, match="images lives on"):
        seg.segment(images, init=("disk", (72, 32, 20)))          # a good start: the next check is the images'


def test_cli_validates_levels(tmp_path):
    cli = os.path.join(ROOT, "bin", "chan_vese")
    img = tmp_path / "a.pgm"
    with open(img, "wb") as f:
        f.write(b"P5\n40 40\n255\n" + bytes(1600))

    def run(*args):
        return subprocess.run([cli, "-i", str(img), "-g", *args], capture_output=True, text=True, timeout=120)

    r = run("--levels", "0")
    assert r.returncode == 1 and "Number of levels must be at least 1: 0." in r.stderr
    r = run("--levels", "-3")
    assert r.returncode == 1 and "Number of levels must be at least 1: -3." in r.stderr
    r = run("--levels", "x")
    assert r.returncode == 1 and "error: the argument ('x') for option '--levels' is invalid" in r.stderr
    r = run("--levels")
    assert r.returncode == 1 and "error: the required argument for option '--levels' is missing" in r.stderr
    r = run("--levels", "2", "--reinit", "5")
    assert r.returncode == 1 and "--reinit" in r.stderr and "--levels" in r.stderr
    r = run("--levels", "2", "--circ", "20,20,5")
    assert r.returncode == 1 and "--circ" in r.stderr and "--levels" in r.stderr
    r = run("--levels", "3")
    assert r.returncode == 1 and "Too many levels for a 40 x 40 image" in r.stderr
    help_text = subprocess.run([cli, "-h"], capture_output=True, text=True, timeout=120).stdout
    assert "--levels arg (=1)" in help_text
    assert "--levels" in open(os.path.join(ROOT, "chan_vese_amd", "host", "main.cpp")).read().split("#include")[0]


def test_the_proposition_on_the_cpu_oracle():
    """Measured on the oracle: 788 iterations in one level; 578 at 64 x 64, 79 at 128 x 128 and 55 at 256 x 256 in three; IoU 0.979.  The
    0.95 is a floor under that number, measured on the reference alone -- not a parity bar."""
    from oracle import cv_oracle as O
    _, (u1, single_steps), levels = U.oracle_proposition()
    fine_steps = levels[0][1]
    score = U.iou_either(O.mask(u1), O.mask(levels[0][0]))
    print("one level:", single_steps, "three levels, finest first:", [s for _, s in levels], "IoU:", score)
    assert fine_steps < single_steps
    assert score >= 0.95
