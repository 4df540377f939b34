"""The tile grid of the resident flow for three channels, on the host (cvh_debug_resident_grid, debug_exports.hip: the arithmetic
resident_geometry() ends in; no device).  Three channels keep three image tiles and three region tables in LDS beside the level set, so
a tile has at most 96 rows (one channel: 128); the largest plane is 256 tiles of 96 x 128."""
import ctypes as C

import pytest

from chan_vese_amd import capi

CAP3 = 96           # rows of a three-channel tile (csv_resident_kernel.hip, rt_hmax)
SMALL = [(16, 16), (16, 128), (32, 256), (48, 130), (96, 160), (96, 128), (130, 258), (200, 384), (256, 1024), (666, 500)]
LARGE = [(1080, 1920), (1536, 2048)]


def grid(h, w, channels, cus=256):
    fn = capi.lib().cvh_debug_resident_grid
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)] * 3
    out = [C.c_int(-1) for _ in range(3)]
    ok = fn(h, w, channels, cus, *[C.byref(o) for o in out])
    return (ok,) + tuple(o.value for o in out)          # (qualifies, tiles_x, tiles_y, rows of the tallest tile)


@pytest.mark.parametrize("shape", SMALL + LARGE)
def test_three_channel_shapes_qualify_and_their_tiles_cover_the_plane(shape):
    h, w = shape
    ok, tx, ty, rows = grid(h, w, 3)
    assert ok == 1, shape
    assert tx * ty <= 256 and tx * 128 >= w and (tx - 1) * 128 < w
    # the kernel deals rows [h t / ty, h (t + 1) / ty) to tile row t: a cover of [0, h) by construction; every tile 16 .. 96 rows
    heights = [(h * (t + 1)) // ty - (h * t) // ty for t in range(ty)]
    assert sum(heights) == h and min(heights) >= 16 and max(heights) <= CAP3 and max(heights) == rows, (shape, ty, heights)


def test_the_largest_three_channel_plane_is_256_tiles_of_96_rows():
    assert grid(1536, 2048, 3) == (1, 16, 16, 96)
    assert grid(1080, 1920, 3) == (1, 15, 17, 64)
    assert grid(1537, 2048, 3)[0] == 0          # one row more than 16 x 96: a tile would need 97 rows
    assert grid(2048, 2048, 3)[0] == 0
    assert grid(1538, 1920, 3) == (1, 15, 17, 91)   # 15 tile columns leave 17 tile rows


def test_one_channel_geometry_did_not_move():
    assert grid(2048, 2048, 1) == (1, 16, 16, 128)
    assert grid(1537, 2048, 1) == (1, 16, 16, 97)
    assert grid(1024, 1024, 1) == (1, 8, 32, 32)
    assert grid(2049, 2048, 1)[0] == 0 and grid(2050, 2048, 1)[0] == 0


@pytest.mark.parametrize("channels", [1, 3])
def test_what_never_qualifies(channels):
    assert grid(512, 511, channels)[0] == 0      # odd width
    assert grid(130, 257, channels)[0] == 0
    assert grid(15, 64, channels)[0] == 0        # fewer than 16 rows / columns
    assert grid(64, 14, channels)[0] == 0
    assert grid(64, 64, 2)[0] == 0               # one or three channels
