"""The restatement of "Mask morphology" (morph_util.py) against facts that do not depend on it: scipy's binary_dilation / binary_erosion
with the header's border values, the duality of erosion and dilation under complement within the plane, open <= F <= close, idempotence
of open and close, the two restatements (shifted ORs, two-pass minimum) against each other, and that the shared cases hold what their
names claim.  CPU only; nothing here touches the library."""
import numpy as np
import pytest

import components_util as CU
import morph_util as M

try:                                                                      # only the comparisons with scipy need it
    from scipy import ndimage
except ImportError:
    ndimage = None

SHAPES = [(1, 1), (1, 70), (33, 257), (65, 300), (3, 8200)]
DENSITIES = (0.02, 0.5, 0.98)
R2S = (0, 1, 2, 4, 5, 9, 25, 100)


def random_plane(h, w, density):
    return np.random.default_rng(int(1000 * density) + 7 * h + w).random((h, w)) < density


def scipy_dilate(f, r2):
    return ndimage.binary_dilation(f, M.disk_structure(r2), border_value=0)


def scipy_erode(f, r2):
    return ndimage.binary_erosion(f, M.disk_structure(r2), border_value=1)


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("h,w", SHAPES)
def test_restatement_obeys_its_laws_and_equals_scipy(h, w, density):
    f = random_plane(h, w, density)
    for r2 in R2S:
        d, e = M.dilate(f, r2), M.erode(f, r2)
        assert np.array_equal(e, ~M.dilate(~f, r2)), r2                       # P \ dilate(P \ F)
        o, c = M.morph(f, M.OPEN, r2), M.morph(f, M.CLOSE, r2)
        if ndimage is not None:                                               # the restatement equals scipy's calls, where scipy imports
            assert np.array_equal(d, scipy_dilate(f, r2)), r2
            assert np.array_equal(e, scipy_erode(f, r2)), r2
            assert np.array_equal(o, scipy_dilate(scipy_erode(f, r2), r2)) and np.array_equal(c, scipy_erode(scipy_dilate(f, r2), r2)), r2
        assert not (o & ~f).any() and not (f & ~c).any(), r2                  # open <= F <= close
        assert np.array_equal(M.morph(o, M.OPEN, r2), o) and np.array_equal(M.morph(c, M.CLOSE, r2), c), r2   # idempotent
        assert np.array_equal(M.morph(f, M.NONE, r2), f)
    assert np.array_equal(M.dilate(f, 0), f) and np.array_equal(M.erode(f, 0), f)


def test_the_small_disks_are_what_the_header_says():
    assert sorted(M.disk_offsets(0)) == [(0, 0)]
    assert sorted(M.disk_offsets(1)) == [(-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)]
    assert M.disk_structure(2).all() and M.disk_structure(2).shape == (3, 3)
    assert len(M.disk_offsets(100)) == 317 and M.isqrt(2 ** 32 - 1) == 65535


@pytest.mark.parametrize("h,w", [(1, 1), (1, 70), (33, 40), (65, 31), (300, 40)])
def test_two_pass_minimum_equals_the_shifts(h, w):
    """the restatement of the large radii against the one scipy was held to, and against brute force over all pairs"""
    for density in ((0.02, 0.5) if h * w <= 4000 else (0.02,)):           # (all pairs: the dense plane only where it is small)
        f = random_plane(h, w, density)
        d2 = M.squared_distance(f)
        pts = np.argwhere(f).astype(np.int64)
        y, x = np.mgrid[0:h, 0:w]
        brute = ((y[..., None] - pts[:, 0]) ** 2 + (x[..., None] - pts[:, 1]) ** 2).min(axis=-1) if len(pts) else np.full((h, w), -1)
        assert np.array_equal(d2, brute)
        for r2 in (1, 5, 25, 100):
            assert np.array_equal((d2 >= 0) & (d2 <= r2), M.dilate_shifts(f, r2)), r2
    assert (M.squared_distance(np.zeros((h, w), bool)) == -1).all()
    assert not M.dilate(np.zeros((h, w), bool), 2 ** 32 - 1).any() and M.erode(np.ones((h, w), bool), 2 ** 32 - 1).all()


def test_the_cases_contain_what_they_claim():
    # a one-pixel bridge that open removes, while the blocks it joins stay
    h, w = 64, 144
    f = M.mask_of(M.case("bridge", h, w))
    row, c0, c1 = M.bridge_geometry(h, w)
    assert f[row, c0:c1].all() and not f[row - 1, c0:c1].any() and not f[row + 1, c0:c1].any()
    o = M.morph(f, M.OPEN, 1)
    assert not o[row, c0 + 1:c1 - 1].any() and o[row, c0 - 2] and o[row, c1 + 1]      # (the bridge's end pixels stay as nubs of the blocks)
    assert CU.label(f, 4)[1].size == 1 and CU.label(o, 4)[1].size == 2     # (components_util's labelling: no scipy)
    # a crack that close fills
    f = M.mask_of(M.case("crack", h, w))
    col, r0, r1 = M.crack_geometry(h, w)
    assert not f[r0:r1, col].any() and f[r0:r1, col - 1].all() and f[r0:r1, col + 1].all()
    assert M.morph(f, M.CLOSE, 1)[r0:r1, col].all()
    # the band seam, rows 31 and 32
    for hh, ww in ((33, 257), (64, 144), (96, 300)):
        f = M.mask_of(M.case("band_seam", hh, ww))
        assert f[31].all() and not f[32].any()
        assert M.dilate(f, 1)[32].all() and not M.erode(f, 1)[31].any() and M.erode(f, 1)[30].all()
    f = M.mask_of(M.case("band_seam", 96, 300))
    assert f[40, 150] and M.dilate(f, 100)[33, 150] and not f[33, 150]
    # the chunk seam, columns 255 and 256
    for hh, ww in ((33, 257), (96, 300)):
        f = M.mask_of(M.case("column_seam", hh, ww))
        assert f[:, 255].all() and not f[:, 256].any()
        assert M.dilate(f, 1)[:, 256].all() and not M.erode(f, 1)[:, 255].any() and M.erode(f, 1)[:, 254].all()
    u = M.case("mask_rule", 64, 144)
    assert np.isnan(u).any() and np.isinf(u).any() and (u == 1e-60).any() and np.signbit(u[u == 0]).any()
    assert not M.mask_of(u)[u == 1e-60].any() and not M.mask_of(u)[np.isnan(u)].any()
    assert M.mask_of(M.case("all_inside", 16, 16)).all() and not M.mask_of(M.case("all_outside", 16, 16)).any()
    # every case exists at every shape, and erosion keeps the border of a full plane (the border rule)
    for hh, ww in M.SHAPES:
        for name in M.CASES:
            assert M.case(name, hh, ww).shape == (hh, ww)
        assert M.expected("all_inside", hh, ww, False, M.ERODE, 25).all() and not M.expected("all_inside", hh, ww, True, M.DILATE, 25).any()
