"""Host logic of the one-buffer flow of the 2-pixel wave kernel (csv_run.hip), on CPU: where one_buffer_rule() takes the flow (reached
through the diagnostic export cvh_debug_one_buffer -- no device needed) and the strips' shadow-row table (one_buffer_table) against a
restatement of what a strip reads of its neighbours."""
import ctypes as C

import numpy as np
import pytest

from chan_vese_amd import capi


def one_buffer(h, w, channels=1, math_mode=2, kernel=-1, state=64, cus=256, live=1, tol=0.0, option=-1):
    fn = capi.lib().cvh_debug_one_buffer
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 8 + [C.c_double, C.c_int]
    r = fn(h, w, channels, math_mode, kernel, state, cus, live, tol, option)
    assert r in (0, 1)
    return r


def test_which_level_set_flow_runs():
    """Automatic choice ("one_buffer" = -1): one buffer only for a single live context whose ping-pong pair exceeds what the Infinity
    Cache holds reliably (~204 MB with the image) while one padded buffer stays below it; everywhere else the pair."""
    assert one_buffer(4096, 4096) == 1                       # 285 MB pair, 160 MB single
    assert one_buffer(2048, 2048) == 0                       # the pair fits (and the resident flow takes the plane)
    assert one_buffer(3000, 4000) == 0                       # 204 MB: the pair still fits
    assert one_buffer(6144, 6144) == 0                       # one buffer does not fit either
    assert one_buffer(4096, 4096, live=2) == 0               # a batch: two live contexts share the cache
    assert one_buffer(4096, 4096, channels=3) == 0
    assert one_buffer(4096, 4096, state=32) == 0
    assert one_buffer(4096, 4096, math_mode=1) == 0          # STRICT arithmetic
    assert one_buffer(4096, 4100) == 0                       # 1-pixel kernel
    assert one_buffer(4096, 4096, tol=1e-3) == 0             # a run that may stop keeps the pair (the iteration beside a stop)
    assert one_buffer(4096, 4096, option=0) == 0
    assert one_buffer(4096, 4096, kernel=3) == 0             # a caller who chose the kernel keeps the flow that choice was made for
    # on request: wherever the flow exists, whatever the footprint
    assert one_buffer(160, 144, kernel=3, option=1) == 0     # (the resident flow may take this plane: "resident" is auto here)
    assert one_buffer(3000, 4000, option=1) == 1 and one_buffer(6144, 6144, option=1) == 1 and one_buffer(4096, 4096, live=2, option=1) == 1
    for kw in (dict(channels=3), dict(state=32), dict(math_mode=1), dict(tol=1e-3)):
        assert one_buffer(4096, 4096, option=1, **kw) == 0, kw
    assert one_buffer(16384, 16368, option=1) == 0            # a slab of 2 GiB or more: 32-bit offsets


def table(b, h):
    fn = capi.lib().cvh_debug_one_buffer_table
    fn.restype = C.c_int
    S = len(b) - 1
    fn.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
    out = (C.c_int * (8 * S))()
    assert fn((C.c_int * (S + 1))(*b), S, h, out) == 0
    return np.array(out[:], dtype=np.int64).reshape(S, 8)


@pytest.mark.parametrize("lengths", [[1, 1, 1, 1, 1], [2, 2, 2, 2, 1], [3, 3, 3, 3, 1], [9, 9, 9, 9, 4], [1, 2, 1, 3, 1, 1, 5], [4, 0, 0, 3, 1, 0, 2],
                                     [0, 1, 1], [7], [1], [5, 1, 1, 1, 6]])
def test_shadow_row_table_feeds_every_reader(lengths):
    """Every strip with rows finds rows max(s0 - 2, 0), s0 - 1 (where s0 > 0) and s1 (where s1 < h) in its three shadow rows: exactly one
    strip publishes each of them, from the right row of its own; nothing else is published."""
    b = np.concatenate([[0], np.cumsum(lengths)]).astype(int)
    h, S = int(b[-1]), len(lengths)
    tab = table(list(b), h)
    want = {}                      # shadow row (strip * 3 + j) -> plane row it must hold
    for k in range(S):
        s0, s1 = b[k], b[k + 1]
        if s1 == s0:
            assert np.all(tab[k] == -1)
            continue
        if s0 > 0:
            want[3 * k] = max(s0 - 2, 0)
            want[3 * k + 1] = s0 - 1
        if s1 < h:
            want[3 * k + 2] = s1
        assert list(tab[k, 5:8]) == [want.get(3 * k, -1), want.get(3 * k + 1, -1), want.get(3 * k + 2, -1)]
    got = {}
    for k in range(S):
        s0, s1 = b[k], b[k + 1]
        for slot, row in ((0, s0), (1, s1 - 1), (2, s1 - 1), (4, s1 - 1), (3, s1 - 2)):
            d = tab[k, slot]
            if d >= 0:
                assert s0 <= row < s1, (k, slot)
                assert d not in got, (k, slot, d)
                got[d] = row
    assert got == want
