"""What the GPU tests of the windowed-plane calls share (test_gpu_local.py, test_gpu_rank.py): the device check behind their capi
fixtures, bit patterns, contexts that do not see each other, plane comparison, a smooth level set, a family's launch-set counter and
the refusal check.  The restatements are local_util's and rank_util's."""
import ctypes

import numpy as np


def device_capi():
    """the body of a module's capi fixture"""
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def alone(ctx, **opts):
    """contexts compared in bits must not see each other in their automatic choices (tests/test_gpu_device_io.py, same_choices)"""
    ctx.set_option("co_resident", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    return ctx


def same_planes(got, want):
    return len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def smooth_levelset(h, w):
    ii, jj = np.mgrid[0:h, 0:w]
    return min(h, w) / 3.0 - np.hypot(ii - h / 2.0, jj - w / 2.0)


def launch_sets(name):
    """launch sets of family `name` ("local", "rank") so far in this process"""
    fn = getattr(ctypes.CDLL(__import__("chan_vese_amd").capi.LIB_PATH), f"cvh_debug_{name}_launch_sets")
    fn.restype = ctypes.c_ulong
    return fn()


def refusal_check(L, unchanged):
    """refused(rc, code, *words, whole=None): the call returned `code`, its message holds every word -- and IS `whole` where given --,
    and unchanged() holds"""
    def refused(rc, code, *words, whole=None):
        assert rc == code
        msg = L.cvh_last_error(None).decode()
        assert all(word in msg for word in words), msg
        assert whole is None or msg == whole, msg
        assert unchanged()
    return refused
