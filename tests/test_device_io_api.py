"""CPU-side checks of the device-memory entry points: declared, exported, bound; the argument errors that are decided before any
device is touched; and torch_io's validation of shapes, dtypes, contiguity and devices, which calls nothing in the library."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cvh_set_image_device", "cvh_get_image_device", "cvh_set_levelset_device", "cvh_get_levelset_device", "cvh_get_mask_device",
         "cvh_set_image_device_batch", "cvh_init_checkerboard_batch", "cvh_get_mask_device_batch"]
ERR_ARG = 1   # CVH_ERR_ARG


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi as m
    return m


def test_header_declares_the_eight_entry_points_and_the_layouts():
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert re.search(r"CVH_LAYOUT_PLANAR\s*=\s*0\s*,\s*CVH_LAYOUT_INTERLEAVED\s*=\s*1", hdr)
    assert re.search(r"cvh_set_image_device_batch\s*\(\s*cvh_context\s*\*\s*const\s*\*\s*ctxs\s*,\s*int\s+n\s*,\s*const\s+uint8_t\s*\*\s*const\s*\*"
                     r"\s*d_imgs\s*,\s*int\s+layout\s*,\s*void\s*\*\s*stream\s*\)", hdr)


def test_library_exports_and_capi_binds_them(capi):
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in capi.EXPORTS
        fn = getattr(capi.lib(), name)
        assert fn.restype is ctypes.c_int and fn.argtypes is not None
    for name in ("set_image_device_batch", "init_checkerboard_batch", "get_mask_device_batch"):
        assert callable(getattr(capi, name))
    for name in ("set_image_device", "get_image_device", "set_levelset_device", "get_levelset_device", "get_mask_device"):
        assert callable(getattr(capi.Context, name))
    assert (capi.LAYOUT_PLANAR, capi.LAYOUT_INTERLEAVED) == (0, 1)


def test_null_context_is_refused_without_a_device(capi):
    L = capi.lib()
    buf = ctypes.c_void_p(0x1000)
    assert L.cvh_set_image_device(None, buf, 0, None) == ERR_ARG
    assert L.cvh_get_image_device(None, buf, 0, None) == ERR_ARG
    assert L.cvh_set_levelset_device(None, buf, 64, None) == ERR_ARG
    assert L.cvh_get_levelset_device(None, buf, 32, None) == ERR_ARG
    assert L.cvh_get_mask_device(None, buf, 0, None) == ERR_ARG
    # (the layout, bits and alignment checks need a live context to be reached: tests/test_gpu_device_io.py,
    # test_single_context_calls_refuse_bad_arguments)


def test_empty_negative_or_null_member_is_refused_without_a_device(capi):
    L = capi.lib()
    ptrs = (ctypes.c_void_p * 2)(0x1000, 0x2000)
    arr = (ctypes.c_void_p * 2)(None, None)
    calls = {
        "cvh_set_image_device_batch": lambda c, n: L.cvh_set_image_device_batch(c, n, ptrs, 0, None),
        "cvh_init_checkerboard_batch": lambda c, n: L.cvh_init_checkerboard_batch(c, n),
        "cvh_get_mask_device_batch": lambda c, n: L.cvh_get_mask_device_batch(c, n, ptrs, 0, None),
    }
    for name, call in calls.items():
        for c, n in ((None, 0), (None, 3), (arr, 0), (arr, -3)):
            assert call(c, n) == ERR_ARG, (name, n)
            msg = L.cvh_last_error(None)
            assert name.encode() in msg and b"member" in msg
        assert call(arr, 2) == ERR_ARG                     # a NULL member
        assert b"member 0 is NULL" in L.cvh_last_error(None)
    for fn in (capi.init_checkerboard_batch, lambda c: capi.set_image_device_batch(c, []), lambda c: capi.get_mask_device_batch(c, [])):
        with pytest.raises(capi.CvhError) as e:
            fn([])
        assert e.value.code == ERR_ARG and "member" in str(e.value)


def test_torch_io_validation_raises_value_error_on_cpu_tensors(capi):
    import torch
    from chan_vese_amd import torch_io
    n, h, w = 2, 8, 12
    good1 = torch.zeros((n, h, w), dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        torch_io.check_images(good1.to(torch.float32), n, h, w, 1)
    with pytest.raises(ValueError, match="torch.Tensor"):
        torch_io.check_images(good1.numpy(), n, h, w, 1)
    for bad in (torch.zeros((n, h, w + 1), dtype=torch.uint8), torch.zeros((n + 1, h, w), dtype=torch.uint8),
                torch.zeros((n, 2, h, w), dtype=torch.uint8), torch.zeros((h, w), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="shape"):
            torch_io.check_images(bad, n, h, w, 1)
    with pytest.raises(ValueError, match="shape"):
        torch_io.check_images(good1, n, h, w, 3)            # (N, H, W) is a one-channel form only
    with pytest.raises(ValueError, match="contiguous"):
        torch_io.check_images(torch.zeros((n, h, 2 * w), dtype=torch.uint8)[:, :, ::2], n, h, w, 1)
    with pytest.raises(ValueError, match="contiguous"):
        torch_io.check_images(torch.zeros((n, h, w, 3), dtype=torch.uint8).permute(0, 3, 1, 2), n, h, w, 3)   # a view, not planar memory
    # well-formed but on the CPU: the device is checked last, so everything above was decided by its own rule
    for t, ch in ((good1, 1), (torch.zeros((n, 3, h, w), dtype=torch.uint8), 3), (torch.zeros((n, h, w, 3), dtype=torch.uint8), 3)):
        with pytest.raises(ValueError, match="lives on cpu"):
            torch_io.check_images(t, n, h, w, ch)
    # members contiguous, batch stride not: accepted as far as the layout rules go (fails on the device rule only)
    with pytest.raises(ValueError, match="lives on cpu"):
        torch_io.check_images(torch.zeros((2 * n, h, w), dtype=torch.uint8)[::2], n, h, w, 1)
    # a shape that is both forms: planar unless told otherwise (decided before the device rule: ask for a layout the shape lacks)
    both = torch.zeros((n, 3, 3, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="lives on cpu"):
        torch_io.check_images(both, n, 3, 3, 3, layout=capi.LAYOUT_INTERLEAVED)
    with pytest.raises(ValueError, match="do not have layout"):
        torch_io.check_images(torch.zeros((n, 3, h, w), dtype=torch.uint8), n, h, w, 3, layout=capi.LAYOUT_INTERLEAVED)
    with pytest.raises(ValueError, match="float64 or float32"):
        torch_io.check_levelsets(torch.zeros((n, h, w), dtype=torch.float16), n, h, w)
    with pytest.raises(ValueError, match="shape"):
        torch_io.check_levelsets(torch.zeros((n, w, h), dtype=torch.float64), n, h, w)
    with pytest.raises(ValueError, match="contiguous"):
        torch_io.check_levelsets(torch.zeros((n, h, 2 * w), dtype=torch.float32)[:, :, ::2], n, h, w)
    with pytest.raises(ValueError, match="lives on cpu"):
        torch_io.check_levelsets(torch.zeros((n, h, w), dtype=torch.float32), n, h, w)
    with pytest.raises(ValueError):
        torch_io.Segmenter(0, h, w)
