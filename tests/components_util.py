"""numpy restatement of the header's "Connected components of the mask" (include/chanvese_hip.h): labelling, table, cleaning.  It is the
checker of tests/test_components_api.py (which holds it against scipy) and tests/test_gpu_components.py; it uses no scipy.

Union-find over the horizontal runs of the mask: a run is a node (numbered in raster order of its first pixel), every vertically -- for
conn = 8 also diagonally -- adjacent pair of foreground pixels an edge between their runs.  Rounds of "hook the larger root onto the
smaller, then compress" (numpy, whole arrays at a time) end with every run pointing at the smallest run of its component, whose first
pixel is the component's smallest flat index."""
import numpy as np

COMPONENT_DTYPE = np.dtype([("first", np.uint32), ("area", np.uint32), ("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32)])


def foreground(u, invert=False):
    """cvh_get_mask's rule: ((float)u > 0) != invert."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        f = np.asarray(u, dtype=np.float64).astype(np.float32) > 0
    return f != bool(invert)


def _compress(parent):
    while True:
        nxt = parent[parent]
        if np.array_equal(nxt, parent):
            return parent
        parent = nxt


def label(mask, conn=4, boxes=True):
    """(labels int32 h x w, table): components numbered 1..K by their smallest flat index; table row k - 1 describes label k.
    boxes = False leaves x0 .. y1 zero (cleaning needs first and area only)."""
    assert conn in (4, 8)
    m = np.asarray(mask).astype(bool)
    h, w = m.shape
    start = m.copy()
    start[:, 1:] &= ~m[:, :-1]
    run = (np.cumsum(start.ravel()) - 1).reshape(h, w)   # the run of a foreground pixel
    nruns = int(start.sum())
    if nruns == 0:
        return np.zeros((h, w), np.int32), np.zeros(0, COMPONENT_DTYPE)
    pairs = [(m[1:, :] & m[:-1, :], (slice(1, None), slice(None)), (slice(0, -1), slice(None)))]
    if conn == 8:
        pairs.append((m[1:, 1:] & m[:-1, :-1], (slice(1, None), slice(1, None)), (slice(0, -1), slice(0, -1))))
        pairs.append((m[1:, :-1] & m[:-1, 1:], (slice(1, None), slice(0, -1)), (slice(0, -1), slice(1, None))))
    a = np.concatenate([run[lo][sel] for sel, lo, up in pairs])
    b = np.concatenate([run[up][sel] for sel, lo, up in pairs])
    if a.size:
        e = np.unique(a.astype(np.int64) * nruns + b)   # every pair of runs once
        a, b = e // nruns, e % nruns
    parent = np.arange(nruns)
    while a.size:
        ra, rb = parent[a], parent[b]
        live = ra != rb
        if not live.any():
            break
        a, b, ra, rb = a[live], b[live], ra[live], rb[live]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))   # a root only ever points at a smaller root
        parent = _compress(parent)
    roots = np.flatnonzero(parent == np.arange(nruns))
    number = np.zeros(nruns, np.int32)
    number[roots] = np.arange(1, roots.size + 1, dtype=np.int32)
    labels = np.where(m, number[parent][run], 0).astype(np.int32)
    flat_start = np.flatnonzero(start.ravel())
    table = np.zeros(roots.size, COMPONENT_DTYPE)
    table["first"] = flat_start[roots]
    rows, cols = np.nonzero(m)
    k = labels[rows, cols] - 1
    table["area"] = np.bincount(k, minlength=roots.size)
    for name, coord, fn, init in () if not boxes else (("x0", cols, np.minimum, w), ("y0", rows, np.minimum, h), ("x1", cols, np.maximum, -1), ("y1", rows, np.maximum, -1)):
        v = np.full(roots.size, init, np.int64)
        fn.at(v, k, coord)
        table[name] = v
    return labels, table


def clean(mask, conn=4, min_area=0, fill_holes=0, keep_largest=False):
    """The header's three steps, in order, on a boolean mask; returns uint8 0/1."""
    m = np.asarray(mask).astype(bool)
    assert min_area >= 0 and fill_holes >= -1
    if min_area > 0:
        lab, tab = label(m, conn, False)
        keep = np.concatenate([[False], tab["area"] >= min_area])
        m = keep[lab]
    if fill_holes != 0:
        lab, tab = label(~m, 8 if conn == 4 else 4, False)
        border = np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))
        hole = np.ones(tab.size + 1, bool)
        hole[border] = False
        hole[0] = False
        if fill_holes > 0:
            hole[1:] &= tab["area"] <= fill_holes
        m = m | hole[lab]
    if keep_largest:
        lab, tab = label(m, conn, False)
        m = (lab == int(np.argmax(tab["area"])) + 1) if tab.size else np.zeros_like(m)   # argmax: the first of equals, the smaller `first`
    return m.astype(np.uint8)


# ---- structured masks the tests share ----
def spiral(h, w):
    """Square rings two pixels apart, each cut below its top-left corner and bridged to the next one inside: one long arm."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.minimum(np.minimum(yy, h - 1 - yy), np.minimum(xx, w - 1 - xx))
    m = (d % 2) == 0
    for k in range(0, min(h, w) // 2, 2):
        if min(h, w) - 2 * k < 5:   # (the innermost ring is too small to cut)
            break
        m[k + 1, k] = False
        if min(h, w) - 2 * (k + 2) >= 1:
            m[k + 2, k + 1] = True
    return m


def comb(h, w):
    """A serpentine: every second row full, joined alternately at the right and the left end -- one component, the longest path."""
    m = np.zeros((h, w), bool)
    m[0::2, :] = True
    for i, r in enumerate(range(1, h, 2)):
        m[r, w - 1 if i % 2 == 0 else 0] = True
    return m


def rings(h, w):
    """Concentric square rings: holes inside holes."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.minimum(np.minimum(yy, h - 1 - yy), np.minimum(xx, w - 1 - xx))
    return (d % 4) == 1


def diagonal(h, w):
    m = np.zeros((h, w), bool)
    i = np.arange(min(h, w))
    m[i, i] = True
    return m


def isolated(h, w):
    m = np.zeros((h, w), bool)
    m[0::2, 0::2] = True
    return m
