"""numpy int64 restatement of the colour-space calls (include/chanvese_hip.h, "Colour spaces"): forward, inverse and luma, the raw
(unclamped) chroma values, the shapes and inputs the tests share, and the proposition's image and its runs on the CPU oracle.  The
definition is in integers, so every comparison against it is an equality.  Shared by test_colour_api.py (CPU), test_gpu_colour.py and
torch_colour_child.py."""
import functools

import numpy as np

H = 8192
D = 128 << 14
SPACES = ["ycrcb", "yuv"]
ORDERS = ["bgr", "rgb"]

# The pixels a workgroup of colour_kernels.hip takes per trip: CVH_BLOCK lanes x one 16-byte piece (cvh_internal.h,
# CVH_COLOUR_BLOCK_PIXELS; test_colour_api.py compares this number with the library's)
BLOCK_PIXELS = 256 * 16
PIECE = 16
# one piece per row and less than a wave (16 x 16); h * w = 323: a partial last piece at an odd byte count (17 x 19); several pieces per
# row and a partial last one (33 x 257); whole pieces only, several waves (64 x 48); one workgroup + one piece of pixels (16 x 257)
SHAPES = [(16, 16), (17, 19), (33, 257), (64, 48), (16, (BLOCK_PIXELS + PIECE) // 16)]
INPUTS = ["random", "all0", "all255", "primaries", "clampers", "greys"]


def _i(a):
    return np.asarray(a, dtype=np.int64)


def _sat(x):
    return np.clip(x, 0, 255)


def _rgb(planes, order):
    p0, p1, p2 = (_i(p) for p in planes)
    if order == "bgr":
        return p2, p1, p0
    if order == "rgb":
        return p0, p1, p2
    raise ValueError(order)


def luma_rgb(r, g, b):
    return (4899 * _i(r) + 9617 * _i(g) + 1868 * _i(b) + H) >> 14


def raw_forward(r, g, b, space):
    """(Y, first chroma, second chroma) BEFORE the clamp, int64"""
    r, g, b = _i(r), _i(g), _i(b)
    y = luma_rgb(r, g, b)
    if space == "ycrcb":
        return y, ((r - y) * 11682 + D + H) >> 14, ((b - y) * 9241 + D + H) >> 14
    if space == "yuv":
        return y, ((b - y) * 8061 + D + H) >> 14, ((r - y) * 14369 + D + H) >> 14
    raise ValueError(space)


def forward(planes, space, order):
    """three uint8 planes in `order` -> [Y, P1, P2] uint8"""
    y, p1, p2 = raw_forward(*_rgb(planes, order), space)
    return [y.astype(np.uint8), _sat(p1).astype(np.uint8), _sat(p2).astype(np.uint8)]


def inverse_rgb(y, p1, p2, space):
    y, a1, a2 = _i(y), _i(p1) - 128, _i(p2) - 128
    if space == "ycrcb":      # a1 = a(Cr), a2 = a(Cb)
        r = y + ((a1 * 22987 + H) >> 14)
        g = y + ((a2 * -5636 + a1 * -11698 + H) >> 14)
        b = y + ((a2 * 29049 + H) >> 14)
    elif space == "yuv":      # a1 = a(U), a2 = a(V)
        r = y + ((a2 * 18678 + H) >> 14)
        g = y + ((a1 * -6472 + a2 * -9519 + H) >> 14)
        b = y + ((a1 * 33292 + H) >> 14)
    else:
        raise ValueError(space)
    return _sat(r), _sat(g), _sat(b)


def inverse(planes, space, order):
    """[Y, P1, P2] uint8 -> three uint8 planes in `order`"""
    r, g, b = (x.astype(np.uint8) for x in inverse_rgb(*planes, space))
    if order == "bgr":
        return [b, g, r]
    if order == "rgb":
        return [r, g, b]
    raise ValueError(order)


def luma(planes, order):
    return luma_rgb(*_rgb(planes, order)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def all_colours():
    """(r, g, b): three int64 arrays of 2^24 entries, every colour once; entry i is r = i >> 16, g = (i >> 8) & 255, b = i & 255.  Shared,
    do not modify."""
    i = np.arange(1 << 24, dtype=np.int64)
    out = (i >> 16, (i >> 8) & 255, i & 255)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def clamp_colours():
    """The (r, g, b) colours that reach each extreme of Y and of the raw chroma values in either space, found by search over all colours."""
    r, g, b = all_colours()
    found = []
    for space in SPACES:
        for v in raw_forward(r, g, b, space):
            for idx in (int(np.argmin(v)), int(np.argmax(v))):
                found.append((int(r[idx]), int(g[idx]), int(b[idx])))
    return sorted(set(found))


def _tile(colours, h, w, order):
    """the colours repeated over an h x w plane in row-major order, as planes in `order`"""
    c = np.asarray(colours, dtype=np.uint8)
    idx = np.arange(h * w) % len(c)
    r, g, b = (c[idx, k].reshape(h, w) for k in range(3))
    return [b, g, r] if order == "bgr" else [r, g, b]


def planes_of(kind, h, w, order="bgr", seed=0):
    """three uint8 planes (h, w) in `order`"""
    from chan_vese_amd import synth
    if kind == "all0":
        return [np.zeros((h, w), dtype=np.uint8) for _ in range(3)]
    if kind == "all255":
        return [np.full((h, w), 255, dtype=np.uint8) for _ in range(3)]
    if kind == "random":
        z = synth.splitmix64_stream(1000 * h + w + seed, 3 * h * w)
        return [(z[k * h * w:(k + 1) * h * w] >> np.uint64(56)).astype(np.uint8).reshape(h, w) for k in range(3)]
    if kind == "primaries":
        return _tile([(255 * (k >> 2), 255 * ((k >> 1) & 1), 255 * (k & 1)) for k in range(8)], h, w, order)
    if kind == "clampers":
        return _tile(clamp_colours(), h, w, order)
    if kind == "greys":
        return _tile([(v, v, v) for v in range(256)], h, w, order)
    raise ValueError(kind)


def every_colour_planes():
    """4096 x 4096 planes (R, G, B) holding every colour once (pixel i is colour i of all_colours)"""
    return [a.astype(np.uint8).reshape(4096, 4096) for a in all_colours()]


def iou(a, b):
    a, b = np.asarray(a) != 0, np.asarray(b) != 0
    union = (a | b).sum()
    return 1.0 if union == 0 else (a & b).sum() / union


def iou_either(a, b):
    """polarity-agnostic: a checkerboard start can converge to either sign"""
    return max(iou(a, b), iou(a, 1 - (np.asarray(b) != 0)))


# ---- the proposition: a reddish disk on a greenish ground of the SAME luma under a left-to-right illumination ramp.  In R, G, B the run
# segments the ramp; in (Y, Cr, Cb) with the luma weighted 0 it finds the disk.
PROP_N = 128
PROP_DISK, PROP_GROUND = (170, 90, 90), (80, 136, 90)      # R, G, B: luma 114 both
PROP_ROWS = [("rgb", (1, 1, 1)), ("ycrcb", (1, 1, 1)), ("ycrcb", (0, 1, 1)), ("ycrcb", (0.05, 1, 1)), ("yuv", (0, 1, 1))]


def proposition_truth(n=PROP_N):
    ii = np.arange(n, dtype=np.int64)[:, None] - n // 2
    jj = np.arange(n, dtype=np.int64)[None, :] - n // 2
    return (ii * ii + jj * jj <= (n // 4) ** 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def proposition_image(n=PROP_N, seed=5):
    """[R, G, B] uint8 planes, integers only: colour x ramp (0.45 .. 1.45 left to right, in 1/1000) + noise per plane and pixel, the sum of
    four uniform integers of -10 .. 10 from synth.splitmix64_stream (sigma = sqrt(4 * 110 / 3) = 12.1, bell-shaped), clamped.  Shared,
    do not modify."""
    from chan_vese_amd import synth
    inside = proposition_truth(n) != 0
    ramp = 450 + (1000 * np.arange(n, dtype=np.int64)) // (n - 1)            # 450 .. 1450
    z = synth.splitmix64_stream(seed, 12 * n * n).reshape(3, 4, n, n)
    planes = []
    for k in range(3):
        base = np.where(inside, PROP_DISK[k], PROP_GROUND[k]).astype(np.int64) * ramp[None, :] // 1000
        noise = sum((z[k, t] % np.uint64(21)).astype(np.int64) - 10 for t in range(4))
        p = np.clip(base + noise, 0, 255).astype(np.uint8)
        p.setflags(write=False)
        planes.append(p)
    return planes


def proposition_planes(space):
    """the planes a row of the table iterates on: the image as (R, G, B), or converted from order "rgb" """
    img = proposition_image()
    return [np.array(p) for p in img] if space == "rgb" else forward(img, space, "rgb")


@functools.lru_cache(maxsize=None)
def oracle_proposition(row):
    """Row `row` of PROP_ROWS on the CPU oracle: checkerboard start, default parameters but lambda1 = lambda2 = the row's weights, 600
    steps at most.  Returns (u, steps, IoU with the disk).  Computed once per process; do not modify."""
    from oracle import cv_oracle as O
    space, lam = PROP_ROWS[row]
    n = PROP_N
    u, steps, _, _ = O.csv_run(proposition_planes(space), O.checkerboard(n, n), O.make_params(lambda1=lam, lambda2=lam), 600, trace=False)
    u.setflags(write=False)
    return u, steps, iou_either(proposition_truth(n), O.mask(u))
