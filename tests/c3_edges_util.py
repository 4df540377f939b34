"""Shapes, inputs, option sets and expected instantiations of tests/test_gpu_c3_edges.py (on the GPU) and tests/test_c3_edges_inputs.py (the
same tables and the oracle's own conditioning, on the CPU): the three-channel 1-pixel wave kernel and tile kernel at the edges of their
geometry, and the aligned-piece image loader (IMGV) of the 1-pixel wave kernel at its threshold widths for one and three channels.

Starts: never the checkerboard.  Its plateaus amplify a 1-ulp perturbation of u0 to 1e-9 of max|u| by iteration 2 (2e-8 by 10 at
37 x 53), so a 1e-9 comparison there measures conditioning.  `normal` and `sdist` keep it below 2e-12 through iteration 10 at every shape
of this file (tests/test_c3_edges_inputs.py asserts the 1e-11 cap, 1/100 of the bar, on the CPU)."""
import numpy as np

STRICT, FAST = 1, 2
MODES = {"strict": STRICT, "fast": FAST}
CHECKPOINTS = (1, 2, 3, 10)
STARTS = ("normal", "sdist")
PARAMS = dict(tol=0, nu=0.01, lambda1=[1, 0.8, 0.5], lambda2=[0.7, 0.5, 1])
BAR = 1e-9          # level set (of max|u|), trace rows (relative): tests/test_gpu_parity.py
COND_CAP = 1e-11    # the oracle's own movement under a 1-ulp perturbation of u0: BAR / 100

# ---- csv_wave_kernel (63 output columns per wave, 4 waves per workgroup, groups of 4 rows), "kernel" = 2; named for the path forced
WAVE_SHAPES = {
    (1, 1): "one pixel", (2, 2): "every clamp", (1, 40): "one row", (40, 1): "one column: lane 1 only",
    (37, 53): "less than one wave column", (5, 63): "exactly one wave column", (6, 64): "a second wave with one column",
    (7, 127): "a third wave with one column", (11, 88): "w >= 80, no multiple of 16: byte loads beside the IMGV threshold",
    (3, 80): "IMGV, below one row group, pieces clamped on both sides of every wave column", (5, 96): "IMGV, one row past a group",
    (4, 112): "IMGV, exactly one group", (13, 128): "IMGV, one row past three groups",
    (17, 1008): "16 x 63: a full last wave, IMGV, 4 workgroups", (33, 256): "IMGV, idle waves in the last workgroup",
    (100, 517): "idle waves, several strips", (3, 700): "12 wave columns, short",
}
IMGV_THRESHOLD = [(3, 80), (5, 96), (4, 112), (13, 128)]
# the shapes the option sets run on: byte loads and aligned pieces, strips that end inside a row group
OPTION_SHAPES = [(37, 53), (11, 88), (100, 517), (3, 80), (13, 128), (33, 256), (17, 1008)]
# (options, modes); every option value meets STRICT and FAST where it exists for both, an IMGV shape and a byte-load shape
WAVE_OPTIONS = {
    "strip8": (dict(strip_rows=8), ("strict", "fast")),
    "strip5": (dict(strip_rows=5), ("strict", "fast")),          # a strip that ends inside a group
    "finalize": (dict(finalize=1), ("strict", "fast")),
    "chain0": (dict(chain=0), ("fast",)),
    "lut0": (dict(lut=0), ("fast",)),
    "pol1": (dict(wave_pol=1), ("fast",)),                       # write-through stores: the <..., 1> instantiation
    "pol0": (dict(wave_pol=0), ("fast",)),                       # (the automatic choice takes write-through for planes this small)
}

# ---- csv_step_kernel (tiles of 256 columns x 14 or 16 rows), "kernel" = 0
TILE_SHAPES = {
    (1, 1): "one pixel", (2, 2): "every clamp", (1, 40): "one row", (40, 1): "one column", (37, 53): "part of a tile, three tile rows",
    (29, 256): "exactly one tile column", (15, 257): "a second tile column of one pixel; 14 / 15 / 16 rows straddle both tile heights",
    (31, 300): "two tile columns",
}
# tile_rows x (mode, lut): the six arithmetic flavours; each also with the LDS-DMA loader ("dma" = 1) on the even widths
TILE_VARIANTS = [(rows, mode, lut) for rows in (14, 16) for mode, lut in (("strict", None), ("fast", 1), ("fast", 0))]


def is_imgv(shape, opts=None):
    return shape[1] % 16 == 0 and shape[1] >= 80 and (opts or {}).get("wave_imgv", 1) != 0


def tf(b):
    return "true" if b else "false"


def wave_name(channels, mode, shape, opts=None, pol=0):
    """The instantiation csv_wave_kernel.hip launches: <C, FAST, LUT, waves per SIMD, IMGV, row groups of 4, store policy>.  pol: the
    store policy the context reports ("wave_pol"); it selects an instantiation of the FAST table flavour only."""
    opts = opts or {}
    fast = mode == "fast"
    lut = fast and opts.get("lut", 1) != 0
    minw = (3 if fast else 2) if channels == 3 else ((5 if lut else 4) if fast else 3)
    return "csv_wave_kernel<%d, %s, %s, %d, %s, 1, %d>" % (channels, tf(fast), tf(lut), minw, tf(is_imgv(shape, opts)),
                                                            pol if lut else 0)


def tile_name(rows, mode, lut, shape, dma):
    """csv_step_kernel<C, tile rows, FAST, LUT, DMA>: the LDS-DMA loader needs an even width and falls back to the register loader."""
    fast = mode == "fast"
    return "csv_step_kernel<3, %d, %s, %s, %s>" % (rows, tf(fast), tf(fast and lut != 0), tf(bool(dma) and shape[1] % 2 == 0))


def tile_options(rows, mode, lut, dma):
    opts = dict(kernel=0, tile_rows=rows)
    if lut is not None:
        opts["lut"] = lut
    if dma:
        opts["dma"] = 1
    return opts


def inputs(shape, start, channels=3):
    """(planes, u0, params): three random planes, then the start, from one generator per shape; one-channel cases use plane 0 and the
    first lambdas."""
    h, w = shape
    rng = np.random.default_rng(h * 7919 + w)
    planes = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)]
    if start == "normal":
        u0 = rng.normal(size=(h, w))
    elif start == "sdist":
        ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        u0 = min(max(h, 3), max(w, 3)) / 3 - np.hypot(ii - h / 2 + 0.3, jj - w / 3 - 0.7)
    else:
        raise ValueError(start)
    pk = dict(PARAMS, lambda1=PARAMS["lambda1"][:channels], lambda2=PARAMS["lambda2"][:channels])
    return planes[:channels], np.ascontiguousarray(u0, dtype=np.float64), pk


_REFERENCE = {}


def reference(oracle, shape, start, channels=3):
    """{"planes", "u0", "pk", "cond": {s: oracle's movement under a 1-ulp perturbation of u0}, "runs": {s: (u, steps_done, trace, mask)}} at
    the four checkpoints; computed once per (shape, start, channels) and shared, read-only, by every option set."""
    key = (shape, start, channels)
    if key not in _REFERENCE:
        from test_gpu_param_edges import conditioned
        planes, u0, pk = inputs(shape, start, channels)
        p = oracle.make_params(**pk)
        runs = {}
        for s in CHECKPOINTS:
            u, done, _, tr = oracle.csv_run(planes, u0, p, s)
            m = oracle.mask(u)
            for a in (u, tr, m):
                a.setflags(write=False)
            runs[s] = (u, done, tr, m)
        u0.setflags(write=False)
        _REFERENCE[key] = dict(planes=planes, u0=u0, pk=pk, cond=conditioned(oracle, planes, u0, pk, CHECKPOINTS), runs=runs)
    return _REFERENCE[key]
