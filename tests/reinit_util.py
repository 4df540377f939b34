"""numpy restatement of level-set reinitialisation (include/chanvese_hip.h, cvh_reinit): the checker of tests/test_reinit_api.py and
tests/test_gpu_reinit.py.  Integers until the final sqrt; written from the header's definition, not from the kernels."""
import numpy as np

NONE = np.iinfo(np.int64).max // 4   # "no pixel of that class in the column" (its square is never formed)


def mask_of(u):
    """cvh_get_mask's rule: NaN, -0.0 and a positive double that rounds to 0.0f are outside."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.asarray(u, dtype=np.float64).astype(np.float32) > 0


def column_pass(m):
    """g[c][i, j] = vertical distance from (i, j) to the nearest pixel of class c in column j (NONE where the column has none), exact,
    by running indices of the last / next row of each class."""
    h, w = m.shape
    rows = np.arange(h, dtype=np.int64)[:, None]
    g = []
    for c in (False, True):
        is_c = m == c
        last = np.maximum.accumulate(np.where(is_c, rows, -1), axis=0)                       # nearest row <= i of class c, or -1
        nxt = np.minimum.accumulate(np.where(is_c, rows, h)[::-1], axis=0)[::-1]            # nearest row >= i of class c, or h
        up = np.where(last >= 0, rows - last, NONE)
        down = np.where(nxt < h, nxt - rows, NONE)
        g.append(np.minimum(up, down))
    return g


def _row_pass_full(f, budget=1 << 24):
    """min over ALL j' of (j - j')^2 + f[row, j'], a few rows at a time"""
    w = f.shape[1]
    cols = np.arange(w, dtype=np.int64)
    dj2 = (cols[:, None] - cols[None, :]) ** 2                                              # [j, j']
    out = np.empty(f.shape, dtype=np.int64)
    chunk = max(1, budget // (w * w))
    for s in range(0, f.shape[0], chunk):
        out[s:s + chunk] = np.min(dj2[None, :, :] + f[s:s + chunk, None, :], axis=2)
    return out


def row_pass(g_other, rows=None, window=64, budget=1 << 24):
    """d2[i, j] = min over j' of (j - j')^2 + g_other[i, j']^2 for the listed rows (all by default): a chunked brute-force minimum.
    To keep large planes affordable the minimum is first taken over |j - j'| <= window only.  That value is an upper bound, and it is
    the exact minimum wherever it is <= (window + 1)^2, because every column outside the window costs at least that much; a row in
    which some pixel exceeds the bound is redone over all columns."""
    h, w = g_other.shape
    rows = np.arange(h) if rows is None else np.asarray(rows)
    g = g_other[rows]
    f = np.where(g >= NONE, NONE, g * g)                                                   # [row, j']
    if window >= w - 1:
        return _row_pass_full(f, budget)
    k = np.arange(-window, window + 1, dtype=np.int64)
    k2 = k * k
    fpad = np.pad(f, ((0, 0), (window, window)), constant_values=NONE)
    out = np.empty(f.shape, dtype=np.int64)
    chunk = max(1, budget // (w * len(k)))
    for s in range(0, len(rows), chunk):
        win = np.lib.stride_tricks.sliding_window_view(fpad[s:s + chunk], len(k), axis=1)   # [row, j, k]
        out[s:s + chunk] = np.min(win + k2[None, None, :], axis=2)
    redo = np.nonzero((out > (window + 1) ** 2).any(axis=1))[0]
    if len(redo):
        out[redo] = _row_pass_full(f[redo], budget)
    return out


def signed_edt(u, rows=None, window=64):
    """(d2 int64, u_new float64, changed) of the level set u.  `rows` restricts the row pass (behind the full column pass) and the
    results to those rows.  A uniform mask: changed is False, u_new is u itself and d2 is zero."""
    u = np.asarray(u, dtype=np.float64)
    m = mask_of(u)
    sel = np.arange(u.shape[0]) if rows is None else np.asarray(rows)
    if m.all() or not m.any():
        return np.zeros((len(sel), u.shape[1]), dtype=np.int64), u[sel].copy(), False
    g0, g1 = column_pass(m)
    msel = m[sel]
    # a pixel of class m needs the distance to class not-m
    d2 = np.where(msel, row_pass(g0, sel, window), row_pass(g1, sel, window))
    d = np.sqrt(d2.astype(np.float64)) - 0.5
    return d2, np.where(msel, d, -d), True


def naive_d2(m):
    """all-pairs minimum, for small masks only"""
    h, w = m.shape
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    pts = np.stack([ii.ravel(), jj.ravel()], 1).astype(np.int64)
    cls = m.ravel()
    d2 = np.zeros(h * w, dtype=np.int64)
    for p in range(h * w):
        other = pts[cls != cls[p]]
        d2[p] = ((other - pts[p]) ** 2).sum(1).min()
    return d2.reshape(h, w)


def bits(a):
    """bit patterns, for == on doubles (NaN payloads and the sign of zero included)"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
