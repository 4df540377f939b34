"""Connected components without a GPU: the numpy restatement (components_util) against scipy and against its own properties, the
exported symbols, and the argument errors the library decides before it touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import components_util as cu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def structured():
    yield "single pixel", np.pad(np.ones((1, 1), bool), 2)
    hole = np.ones((5, 5), bool)
    hole[2, 2] = False
    yield "single hole", hole
    yield "diagonal pair", np.eye(2, dtype=bool)
    yield "1xN", np.arange(17)[None, :] % 3 != 0
    yield "Nx1", np.arange(17)[:, None] % 3 != 0
    yield "2x2", np.ones((2, 2), bool)
    yield "rings", cu.rings(23, 24)
    yield "spiral", cu.spiral(21, 24)
    yield "comb", cu.comb(19, 11)
    yield "all foreground", np.ones((6, 7), bool)
    yield "all background", np.zeros((6, 7), bool)
    open_hole = np.ones((5, 5), bool)
    open_hole[2, 0:3] = False
    yield "hole touching the border", open_hole


def random_masks():
    rng = np.random.default_rng(11)
    for density in (0.3, 0.5, 0.6, 0.8):
        for _ in range(40):
            h, w = rng.integers(1, 25, 2)
            yield f"random {h}x{w} at {density}", rng.random((h, w)) < density


@pytest.mark.parametrize("conn", [4, 8])
def test_restatement_against_scipy(conn):
    ndi = pytest.importorskip("scipy.ndimage")
    cross, full = ndi.generate_binary_structure(2, 1), np.ones((3, 3))
    s, sc = (cross, full) if conn == 4 else (full, cross)
    for name, m in list(structured()) + list(random_masks()):
        labels, table = cu.label(m, conn)
        want, k = ndi.label(m, s)
        assert k == table.size and np.array_equal(labels, want), name
        assert np.array_equal(cu.clean(m, conn, 0, -1, False).astype(bool), ndi.binary_fill_holes(m, sc)), name


def test_structured_counts():
    m = dict(structured())
    assert cu.label(m["diagonal pair"], 4)[1].size == 2 and cu.label(m["diagonal pair"], 8)[1].size == 1
    assert cu.label(m["comb"], 4)[1].size == 1 and cu.label(m["spiral"], 4)[1].size == 1
    assert cu.label(m["all background"], 4)[1].size == 0 and not cu.clean(m["all background"], 4, 0, -1, True).any()
    assert cu.clean(m["single hole"], 4, 0, -1).all() and cu.clean(m["single hole"], 4, 0, 1).all()
    assert np.array_equal(cu.clean(m["hole touching the border"], 4, 0, -1), m["hole touching the border"])
    ring = cu.rings(23, 24)
    assert cu.clean(ring, 4, 0, -1)[1:-1, 1:-1].all()   # holes inside holes: everything inside the outer ring


@pytest.mark.parametrize("conn", [4, 8])
def test_restatement_properties(conn):
    for name, m in list(structured()) + list(random_masks()):
        labels, t = cu.label(m, conn)
        h, w = m.shape
        assert np.all(np.diff(t["first"].astype(np.int64)) > 0), name
        seen = labels.ravel()[labels.ravel() > 0]
        order = seen[np.sort(np.unique(seen, return_index=True)[1])]
        assert np.array_equal(order, np.arange(1, t.size + 1)), name          # labels appear in raster order
        assert np.array_equal(labels.ravel()[t["first"]], np.arange(1, t.size + 1)), name
        assert int(t["area"].sum()) == int(m.sum()), name
        rows, cols = np.nonzero(m)
        r = t[labels[rows, cols] - 1]
        assert np.all((r["x0"] <= cols) & (cols <= r["x1"]) & (r["y0"] <= rows) & (rows <= r["y1"])), name
        assert np.array_equal(cu.clean(m, conn, 0, 0, False), m.astype(np.uint8)), name


def test_keep_largest_tie_goes_to_smaller_first():
    m = np.zeros((5, 9), bool)
    m[1:3, 1:3] = True
    m[2:4, 5:7] = True
    out = cu.clean(m, 4, 0, 0, True)
    assert out[1:3, 1:3].all() and out.sum() == 4


def test_symbols_exported():
    from chan_vese_amd import capi
    L = capi.lib()
    for name in ("cvh_components", "cvh_components_batch", "cvh_get_mask_clean", "cvh_get_mask_clean_device", "cvh_get_mask_clean_device_batch"):
        assert name in capi.EXPORTS and hasattr(L, name)
    assert capi.COMPONENT_DTYPE == cu.COMPONENT_DTYPE and capi.COMPONENT_DTYPE.itemsize == 24


def test_argument_errors_before_any_device():
    """what a batch call decides from its member list alone"""
    from chan_vese_amd import capi
    L = capi.lib()
    none = (C.c_void_p * 1)(None)
    for call in (lambda a, n: L.cvh_components_batch(a, n, 4, 0, None, None, None),
                 lambda a, n: L.cvh_get_mask_clean_device_batch(a, n, None, 4, 0, 3, 0, 0, None)):
        assert call(None, 1) == 1 and b"empty member list" in L.cvh_last_error(None)
        assert call(none, 0) == 1 and b"empty member list" in L.cvh_last_error(None)
        assert call(none, 1) == 1 and b"member 0 is NULL" in L.cvh_last_error(None)
    assert L.cvh_components(None, 4, 0, None, None, 0, None, None) == 1
    assert L.cvh_get_mask_clean(None, None, 4, 0, 0, 0, 0) == 1
    assert L.cvh_get_mask_clean_device(None, None, 4, 0, 0, 0, 0, None) == 1


def test_parameter_errors_before_any_device():
    """conn, min_area, fill_holes and keep_largest are decided behind the member list and before the device is touched: with a NULL
    member the list fails first, so the order is visible without a context -- and with a real one in tests/test_gpu_components.py"""
    from chan_vese_amd import capi
    L = capi.lib()
    none = (C.c_void_p * 1)(None)
    assert L.cvh_get_mask_clean_device_batch(none, 1, None, 4, 0, -1, 0, 0, None) == 1 and b"member 0 is NULL" in L.cvh_last_error(None)
    for args in ((5, 0, 0, 0, 0), (4, 0, -1, 0, 0), (4, 0, 0, -2, 0), (4, 0, 0, 0, 2)):
        assert L.cvh_get_mask_clean(None, None, *args) == 1
        assert L.cvh_get_mask_clean_device(None, None, *args, None) == 1


def test_cli_validation_messages(tmp_path):
    cli = os.path.join(ROOT, "bin", "chan_vese")
    img = tmp_path / "a.pgm"
    with open(img, "wb") as f:
        f.write(b"P5\n8 8\n255\n" + bytes(64))
    for flags, msg in ((["--min-area", "-1"], "Minimum component area cannot be negative: -1."),
                       (["--fill-holes", "-2"], "Largest hole to fill must be -1 (any size), zero or positive: -2."),
                       (["--connectivity", "6"], "Connectivity must be 4 or 8: 6."),
                       (["--connectivity", "x"], "error: the argument ('x') for option '--connectivity' is invalid"),
                       (["--min-area", "1.5"], "error: the argument ('1.5') for option '--min-area' is invalid"),
                       (["--fill-holes"], "error: the required argument for option '--fill-holes' is missing"),
                       (["--largest=1"], "error: option '--largest' does not take any arguments")):
        r = subprocess.run([cli, "-i", str(img)] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and msg in r.stderr, (flags, r.stderr)
    out = subprocess.run([cli, "-h"], capture_output=True, text=True, timeout=120).stdout
    for flag in ("--connectivity", "--min-area", "--fill-holes", "--largest", "--roi"):
        assert flag in out
