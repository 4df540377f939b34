"""ctypes binding of include/chanvese_hip.h (the C ABI of libchanvese_hip.so).

No CPU fallback: if the HIP library has not been built, importing/using this module raises
with instructions.  In a process that also imports torch, import torch FIRST: torch ships
its own libamdhip64.so.7 and the loader then shares that one runtime with this library.
"""
import ctypes as C
import dataclasses
import math

import numpy as np

from ._abi import (COLOUR_SPACES, COMPONENT_DTYPE, CONTOUR_LOOP_DTYPE, CVH_OK, EXPORTS, LAYOUT_INTERLEAVED, LAYOUT_PLANAR, LIB_PATH, LOCAL_COPY, LOCAL_DEV,
                   LOCAL_MEAN, LOCAL_RADIUS_MAX, LOCAL_WHATS, MATH_DEFAULT, MATH_FAST, MATH_STRICT, MORPH_CLOSE, MORPH_DILATE, MORPH_ERODE, MORPH_NONE,
                   MORPH_OPEN, MORPH_OPS, OP_DELTA, OP_HEAVISIDE, OP_ONE_MINUS_HEAVISIDE, ORDERS, OVERLAP_DTYPE, RANK_BOTHAT, RANK_CLOSE, RANK_COPY, RANK_MAX,
                   RANK_MEDIAN, RANK_MEDIAN_RADIUS_MAX, RANK_MIN, RANK_OPEN, RANK_RADIUS_MAX, RANK_TOPHAT, RANK_WHATS, REGION_DTYPE, REGION_SHAPE_DTYPE,
                   SIGNATURES, SMOOTH_BLUR, SMOOTH_COPY, SMOOTH_DETAIL, SMOOTH_RADIUS_MAX, SMOOTH_TAP_SUM, SMOOTH_WHATS, ConvexParams, CvhError, EnergyTerms, MaskScore, Match, Params, lib)


@dataclasses.dataclass(frozen=True)
class Energy:
    """The Chan-Sandberg-Vese functional of a context's current level set, term by term: total = mu length + nu area +
    (1/C) sum_k (lambda1_k fit_in[k] + lambda2_k fit_out[k]); the tuples hold one entry per channel, c1 / c2 the means the fit terms
    were taken with (Context.get_means)."""
    total: float
    length: float
    area: float
    fit_in: tuple
    fit_out: tuple
    c1: tuple
    c2: tuple


def _energy_of(t, channels):
    return Energy(t.total, t.length, t.area, *(tuple(getattr(t, f)[k] for k in range(channels)) for f in ("fit_in", "fit_out", "c1", "c2")))


SCORE_FIELDS = tuple(f for f, _ in MaskScore._fields_ if f != "pad")


def _ratio(num, den):
    return num / den if den else math.nan


@dataclasses.dataclass(frozen=True)
class Score:
    """A mask against a ground truth ("Mask scores" in include/chanvese_hip.h): the exact integers of cvh_mask_score, and the figures the
    header derives from them -- each NaN where its denominator is 0 or, for the boundary measures, where a surface is empty."""
    tp: int
    fp: int
    fn: int
    tn: int
    surf_m: int
    surf_t: int
    within_m: int
    within_t: int
    dist_m_q16: int
    dist_t_q16: int
    hd2_m: int
    hd2_t: int
    defined: int

    @property
    def iou(self):
        return _ratio(self.tp, self.tp + self.fp + self.fn)

    @property
    def dice(self):
        return _ratio(2 * self.tp, 2 * self.tp + self.fp + self.fn)

    @property
    def hausdorff(self):
        return math.sqrt(max(self.hd2_m, self.hd2_t)) if self.defined else math.nan

    @property
    def assd(self):
        return _ratio((self.dist_m_q16 + self.dist_t_q16) / 65536, self.surf_m + self.surf_t) if self.defined else math.nan

    @property
    def surface_dice(self):
        return _ratio(self.within_m + self.within_t, self.surf_m + self.surf_t) if self.defined else math.nan


@dataclasses.dataclass(frozen=True)
class ObjectScore:
    """The components of a mask against a set of objects ("Component overlaps" in include/chanvese_hip.h): the exact integers of
    cvh_match at one IoU threshold, the figures the header derives from them -- each NaN where its denominator is 0 --, and, where
    match_overlaps took them, tp at the thresholds 10/20 .. 19/20 for mean_ap."""
    objects_a: int
    objects_b: int
    tp: int
    fp: int
    fn: int
    tp_at: tuple = ()

    @property
    def precision(self):
        return _ratio(self.tp, self.tp + self.fp)

    @property
    def recall(self):
        return _ratio(self.tp, self.tp + self.fn)

    @property
    def f1(self):
        return _ratio(2 * self.tp, 2 * self.tp + self.fp + self.fn)

    @property
    def ap(self):
        return _ratio(self.tp, self.tp + self.fp + self.fn)

    @property
    def mean_ap(self):
        """the mean over num / den = 10/20 .. 19/20 of tp / (tp + fp + fn); NaN without objects on either side, or without tp_at"""
        total = self.objects_a + self.objects_b
        if len(self.tp_at) != 10 or not total:
            return math.nan
        return sum(t / (total - t) for t in self.tp_at) / 10


def _score_of(s):
    return Score(*(int(getattr(s, f)) for f in SCORE_FIELDS))


def score_tol2(tol):
    """The squared tolerance the score calls take: floor(tol^2) for a finite tol >= 0, capped at 2^32 - 1."""
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not math.isfinite(tol) or tol < 0:
        raise ValueError(f"tol must be a finite number >= 0, got {tol!r}")
    return min(int(math.floor(tol * tol)), 0xFFFFFFFF)


def r2_of(radius):
    """The squared radius the morphology calls take: floor(radius^2) for a finite radius >= 0, capped at 2^32 - 1."""
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not math.isfinite(radius) or radius < 0:
        raise ValueError(f"radius must be a finite number >= 0, got {radius!r}")
    return min(int(math.floor(radius * radius)), 0xFFFFFFFF)


def morph_code(op):
    """CVH_MORPH_*: from its code or from "none" / "dilate" / "erode" / "open" / "close" (None is "none")"""
    if op is None:
        return MORPH_NONE
    if isinstance(op, str):
        if op.lower() not in MORPH_OPS:
            raise ValueError(f"morph must be one of {sorted(MORPH_OPS)}, got {op!r}")
        return MORPH_OPS[op.lower()]
    return int(op)


def _morph_r2(r2, radius):
    """the one squared radius of a call: r2 (an integer 0 .. 2^32 - 1) or radius (r2_of), not both; neither is 0"""
    if r2 is not None and radius is not None:
        raise ValueError("give r2 or radius, not both")
    if radius is not None:
        return r2_of(radius)
    r2 = 0 if r2 is None else int(r2)
    if not 0 <= r2 <= 0xFFFFFFFF:
        raise ValueError(f"r2 must be in 0 .. 2^32 - 1, got {r2}")
    return r2


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


# ---- the marshalling idioms, once each: a new wrapper uses these and spells none of them out
def _ptr(x):
    """a device address or a stream handle, held as an integer, as a void * argument: 0 is NULL"""
    return int(x) or None


def _array(ctype, n, values=()):
    """a ctypes array of n entries -- of one where n is 0, so that an empty batch still hands the library an address"""
    return (ctype * max(n, 1))(*values)


def _member_array(contexts):
    return _array(C.c_void_p, len(contexts), [c._h.value for c in contexts])


def _members(contexts):
    """(the members as a list, n); their handles are read by _member_array in the call itself, behind every check of the other arguments"""
    contexts = list(contexts)
    return contexts, len(contexts)


def _address_array(ptrs, n):
    ptrs = list(ptrs)
    if len(ptrs) != n:
        raise ValueError(f"{len(ptrs)} device pointers for {n} members")
    return _array(C.c_void_p, n, [_ptr(p) for p in ptrs])


def _per_member(value, n, name, conv, ndim=0):
    """[conv(v)] per member: `value` is one value for all members (an array of `ndim` dimensions, 0 = a scalar) or a sequence of exactly n"""
    vals = list(value) if np.ndim(value) > ndim else [value] * n
    if len(vals) != n:
        raise ValueError(f"{name}: {len(vals)} values for {n} members")
    return [conv(v) for v in vals]


def _check(rc):
    """raises on an error code of a call that leaves its message with the thread (cvh_last_error(NULL)); Context._chk reads the context's"""
    if rc != CVH_OK:
        raise CvhError(rc, lib().cvh_last_error(None).decode())


def _table_pointers(tables, n):
    return _array(C.c_void_p, n, [t.ctypes.data if t.size else None for t in tables])


def _rows(call, dtype, cap):
    """One call for the first rows of a table: call(table_pointer, cap) makes the library call and returns the count it reports.
    Returns (count, the first min(count, cap) rows)."""
    table = np.zeros(max(int(cap), 0), dtype=dtype)
    count = call(table.ctypes.data if table.size else None, int(cap))
    return count, table[:min(count, table.size)].copy()


def _count_then_rows(call, dtype, cap):
    """_rows, and for cap = None every row at the price of a first call(None, 0) for the count: the host table must exist before the call
    that fills it.  No rows: no second call."""
    if cap is None:
        cap = call(None, 0)
        if not cap:
            return 0, np.zeros(0, dtype=dtype)
    return _rows(call, dtype, cap)


def _caps_batch(call, cap, n, name):
    """the row capacities of a batch: cap is one number for every member or one per member, or None for the counts a first
    call(None, None) reports"""
    return call(None, None) if cap is None else _per_member(cap, n, name, int)


def _rows_batch(call, dtype, caps, ctype):
    """_rows for a batch: call(table_pointers, caps) makes the library call and returns the members' counts; caps as a ctypes array of
    `ctype`.  Returns [the first min(count, cap) rows] per member."""
    n = len(caps)
    tables = [np.zeros(max(c, 0), dtype=dtype) for c in caps]
    counts = call(_table_pointers(tables, n), _array(ctype, n, caps))
    return [t[:min(k, t.size)].copy() for k, t in zip(counts, tables)]


def make_params(mu=0.5, nu=0.0, dt=1.0, eps=1.0, tol=1e-3, lambda1=None, lambda2=None):
    p = Params()
    lib().cvh_default_params(C.byref(p))
    p.mu, p.nu, p.dt, p.eps, p.tol = mu, nu, dt, eps, tol
    for name, vals in (("lambda1", lambda1), ("lambda2", lambda2)):
        if vals is not None:
            arr = getattr(p, name)
            for k, v in enumerate(vals):
                arr[k] = float(v)
    return p


def device_count():
    n = C.c_int(0)
    lib().cvh_device_count(C.byref(n))
    return n.value


def pm_trip_count(L, T):
    return lib().cvh_pm_trip_count(float(L), float(T))


def checkerboard_host(h, w):
    u = np.empty((h, w), dtype=np.float64)
    lib().cvh_levelset_checkerboard_host(h, w, _dp(u))
    return u


def ppf_apply(data, op, eps=1.0, start=0, end=None, device=0):
    """ParallelPixelFunction(data, w, f)(Range(start, end)) on the GPU, in place."""
    assert data.dtype == np.float64 and data.flags.c_contiguous and data.ndim == 2
    end = data.size if end is None else end
    _check(lib().cvh_ppf_apply(_dp(data), data.shape[1], start, end, int(op), float(eps), device))
    return data


def enqueue_steps_batch(contexts, n):
    """Fused batch (cvh_enqueue_steps_batch): enqueues n iterations of every context with one launch per iteration and
    CSV-step instantiation; follow with sync() on each context, as after Context.enqueue_steps."""
    contexts = list(contexts)
    rc = lib().cvh_enqueue_steps_batch(_member_array(contexts), len(contexts), int(n))
    if rc != CVH_OK:   # (tested here: the timed path gains no call where the library succeeds)
        _check(rc)


def run_batch(contexts, max_steps=-1):
    """Fused batch (cvh_run_batch): Context.run for every context at once, each with its own stop rule.
    Returns [(steps_done, last_norm)] per context."""
    contexts = list(contexts)
    n = len(contexts)
    done, nrm = (C.c_int * max(n, 1))(), (C.c_double * max(n, 1))()
    rc = lib().cvh_run_batch(_member_array(contexts), n, int(max_steps), done, nrm)
    if rc != CVH_OK:   # (as in enqueue_steps_batch)
        _check(rc)
    return [(done[i], nrm[i]) for i in range(n)]


def perona_malik_batch(contexts, K=10.0, L=0.25, T=20.0):
    """Perona-Malik batch (cvh_perona_malik_batch): Context.perona_malik for every context at once, the planes of several
    contexts sharing resident launches.  K, L and T are scalars (the same for every member) or sequences of one value per member."""
    contexts, n = _members(contexts)
    k, l, t = (_array(C.c_double, n, _per_member(v, n, name, float)) for v, name in ((K, "K"), (L, "L"), (T, "T")))
    _check(lib().cvh_perona_malik_batch(_member_array(contexts), n, k, l, t))


def set_image_device_batch(contexts, ptrs, layout=LAYOUT_PLANAR, stream=0):
    """cvh_set_image_device_batch: every context takes its image from device memory (ptrs: one integer address per context, uint8,
    planar or interleaved), one launch for all; ordered behind what `stream` (a HIP stream handle as integer, 0 = default) holds."""
    contexts, n = _members(contexts)
    _check(lib().cvh_set_image_device_batch(_member_array(contexts), n, _address_array(ptrs, n), int(layout), _ptr(stream)))


def init_checkerboard_batch(contexts):
    """cvh_init_checkerboard_batch: Context.init_checkerboard for every context with one copy and one launch."""
    contexts, n = _members(contexts)
    _check(lib().cvh_init_checkerboard_batch(_member_array(contexts), n))


def get_mask_device_batch(contexts, ptrs, invert=False, stream=0):
    """cvh_get_mask_device_batch: every context's mask into device memory (ptrs: one integer address of h * w bytes per context),
    one launch for all; work enqueued on `stream` afterwards sees the masks.  Does not block the host."""
    contexts, n = _members(contexts)
    _check(lib().cvh_get_mask_device_batch(_member_array(contexts), n, _address_array(ptrs, n), int(bool(invert)), _ptr(stream)))


def reinit_batch(contexts):
    """cvh_reinit_batch: Context.reinit for every context (any mix of shapes) with one set of launches.  Returns [changed] per context."""
    contexts, n = _members(contexts)
    changed = _array(C.c_int, n)
    _check(lib().cvh_reinit_batch(_member_array(contexts), n, changed))
    return [bool(changed[i]) for i in range(n)]


def components_batch(contexts, ptrs=None, conn=4, invert=False, stream=0):
    """cvh_components_batch: the connected components of every context's mask with one set of launches.  ptrs: one integer device
    address of h * w int32 labels per context (0 = no label plane for that member), or None.  Returns [K] per context."""
    contexts, n = _members(contexts)
    counts = _array(C.c_int, n)
    addr = None if ptrs is None else _address_array(ptrs, n)
    _check(lib().cvh_components_batch(_member_array(contexts), n, int(conn), int(bool(invert)), addr, counts, _ptr(stream)))
    return [counts[i] for i in range(n)]


def get_mask_clean_device_batch(contexts, ptrs, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, stream=0):
    """cvh_get_mask_clean_device_batch: every context's cleaned mask (Context.get_mask_clean) into device memory, one set of launches
    for all; work enqueued on `stream` afterwards sees the masks.  Does not block the host."""
    contexts, n = _members(contexts)
    _check(lib().cvh_get_mask_clean_device_batch(_member_array(contexts), n, _address_array(ptrs, n), int(conn), int(bool(invert)),
                                                     int(min_area), int(fill_holes), int(keep_largest), _ptr(stream)))


def otsu_from_histogram(hist):
    """cvh_otsu_from_histogram: Otsu's threshold of a histogram of 1 .. 766 uint32 counts (the header's integer definition), on the host."""
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    t = C.c_int(-1)
    _check(lib().cvh_otsu_from_histogram(hist.ctypes.data, int(hist.size), C.byref(t)))
    return t.value


def _int_rows(values, n, width, name):
    """values: one row of `width` ints for all members, or a sequence of n rows -> a flat ctypes int array of n * width"""
    flat = []
    for r in _per_member(values, n, name, lambda r: [r] if width == 1 else list(r), ndim=int(width > 1)):
        if len(r) != width:
            raise ValueError(f"{name}: {len(r)} numbers where {width} are needed")
        flat += [int(v) for v in r]
    return _array(C.c_int, len(flat), flat)


def histogram_batch(contexts, caps=None):
    """cvh_histogram_batch: the grey histograms (g = the sum of the planes) of every context with one launch.  caps: bins wanted per
    member (None: all 255 C + 1).  Returns [uint32 array] per context."""
    contexts, n = _members(contexts)
    caps = [255 * c.channels + 1 for c in contexts] if caps is None else _per_member(caps, n, "caps", int)
    outs = [np.zeros(max(k, 0), dtype=np.uint32) for k in caps]
    _check(lib().cvh_histogram_batch(_member_array(contexts), n, _table_pointers(outs, n), _array(C.c_int, n, caps)))
    return [o[:min(o.size, 255 * c.channels + 1)] for o, c in zip(outs, contexts)]


def init_threshold_batch(contexts, t, inside=1.0, outside=-1.0):
    """cvh_init_threshold_batch: Context.init_threshold for every context with one launch; t is one int or one per member."""
    contexts, n = _members(contexts)
    _check(lib().cvh_init_threshold_batch(_member_array(contexts), n, _int_rows(t, n, 1, "t"), float(inside), float(outside)))


def init_otsu_batch(contexts, inside=1.0, outside=-1.0):
    """cvh_init_otsu_batch: Context.init_otsu for every context: one histogram launch, one start launch.  Returns [t] per context."""
    contexts, n = _members(contexts)
    t = _array(C.c_int, n)
    _check(lib().cvh_init_otsu_batch(_member_array(contexts), n, t, float(inside), float(outside)))
    return [t[i] for i in range(n)]


def init_rect_batch(contexts, xywh, inside=1.0, outside=0.0):
    """cvh_init_rect_batch: Context.init_rect for every context with one launch; xywh is (x, y, w, h) or one such row per member."""
    contexts, n = _members(contexts)
    _check(lib().cvh_init_rect_batch(_member_array(contexts), n, _int_rows(xywh, n, 4, "xywh"), float(inside), float(outside)))


def init_disk_batch(contexts, cxcyr, inside=1.0, outside=0.0):
    """cvh_init_disk_batch: Context.init_disk for every context with one launch; cxcyr is (cx, cy, r) or one such row per member."""
    contexts, n = _members(contexts)
    _check(lib().cvh_init_disk_batch(_member_array(contexts), n, _int_rows(cxcyr, n, 3, "cxcyr"), float(inside), float(outside)))


def pyramid_shapes(h, w, levels):
    """The shapes of a pyramid of `levels` levels over an h x w plane, finest first: [(h, w), ((h + 1) // 2, (w + 1) // 2), ...].
    ValueError when levels < 1 or when the coarsest side would fall below 16.  Calls nothing in the library."""
    if levels < 1:
        raise ValueError(f"levels must be >= 1, got {levels}")
    shapes = [(int(h), int(w))]
    for _ in range(levels - 1):
        shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2))
    if min(shapes[-1]) < 16:
        raise ValueError(f"{levels} levels over {h} x {w} end at {shapes[-1][0]} x {shapes[-1][1]}: the coarsest side must not fall below 16")
    return shapes


def _pairs(a, b):
    a, b = list(a), list(b)
    if len(a) != len(b):
        raise ValueError(f"{len(a)} and {len(b)} contexts do not pair up")
    return a, b


def restrict_image_batch(fines, coarses):
    """cvh_restrict_image_batch: Context.restrict_image_to for n pairs (any mix of shapes and channel counts) with one launch."""
    fines, coarses = _pairs(fines, coarses)
    _check(lib().cvh_restrict_image_batch(_member_array(fines), _member_array(coarses), len(fines)))


def prolong_levelset_batch(coarses, fines):
    """cvh_prolong_levelset_batch: Context.prolong_levelset_to for n pairs (any mix of shapes and channel counts) with one launch."""
    coarses, fines = _pairs(coarses, fines)
    _check(lib().cvh_prolong_levelset_batch(_member_array(coarses), _member_array(fines), len(coarses)))


def colour_space_code(space):
    """"ycrcb" / "yuv" -> CVH_COLOUR_*; ValueError for anything else.  Calls nothing in the library."""
    if not isinstance(space, str) or space.lower() not in COLOUR_SPACES:
        raise ValueError(f"colour space must be one of {sorted(COLOUR_SPACES)}, got {space!r}")
    return COLOUR_SPACES[space.lower()]


def order_code(order):
    """"bgr" / "rgb" -> CVH_ORDER_*; ValueError for anything else.  Calls nothing in the library."""
    if not isinstance(order, str) or order.lower() not in ORDERS:
        raise ValueError(f"plane order must be one of {sorted(ORDERS)}, got {order!r}")
    return ORDERS[order.lower()]


def convert_colour_batch(contexts, space, order="bgr", inverse=False):
    """cvh_convert_colour_batch: Context.convert_colour for n three-channel contexts (any mix of shapes) with one launch."""
    space, order = colour_space_code(space), order_code(order)
    contexts, n = _members(contexts)
    _check(lib().cvh_convert_colour_batch(_member_array(contexts), n, space, order, int(bool(inverse))))


def luma_image_batch(srcs, dsts, order="bgr"):
    """cvh_luma_image_batch: Context.luma_to for n pairs (any mix of shapes) with one launch."""
    order = order_code(order)
    srcs, dsts = _pairs(srcs, dsts)
    _check(lib().cvh_luma_image_batch(_member_array(srcs), _member_array(dsts), len(srcs), order))


def _what_codes(what, kind, names, top, range_text):
    """A name out of `names` or 1 to 3 codes 0 .. top -> three codes, filled with 0 (the copy)."""
    if isinstance(what, str):
        if what.lower() not in names:
            raise ValueError(f"{kind} must be one of {sorted(names)} or a tuple of codes, got {what!r}")
        named = names[what.lower()]
        return named if isinstance(named, tuple) else (named,) * 3
    try:
        codes = tuple(what)
    except TypeError:
        codes = None
    if not codes or len(codes) > 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= top for v in codes):
        raise ValueError(f"{kind} must be one of {sorted(names)} or 1 to 3 codes out of {range_text}, got {what!r}")
    return tuple(int(v) for v in codes) + (0,) * (3 - len(codes))


def _radius(radius, kind, top, note=""):
    """An integer 0 .. top."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= top:
        raise ValueError(f"{kind} radius must be an integer 0 .. {top}{note}, got {radius!r}")
    return int(radius)


def local_what_codes(what):
    """A name -- "mean", "dev" (every plane) or "stack" (copy, mean, deviation) -- or 1 to 3 codes -> the three codes cvh_local_planes
    reads; entries a destination has no plane for are ignored by the library and filled with LOCAL_COPY here.  ValueError for anything
    else.  Calls nothing in the library."""
    return _what_codes(what, "local statistic", LOCAL_WHATS, LOCAL_DEV, "LOCAL_COPY (0), LOCAL_MEAN (1), LOCAL_DEV (2)")


def local_radius(radius):
    """An integer 0 .. LOCAL_RADIUS_MAX; ValueError for anything else.  Calls nothing in the library."""
    return _radius(radius, "local", LOCAL_RADIUS_MAX)


def rank_what_codes(what):
    """A name -- "min", "max", "median", "open", "close", "tophat", "bothat" (every plane) -- or 1 to 3 codes -> the three codes
    cvh_rank_planes reads; entries a destination has no plane for are ignored by the library and filled with RANK_COPY here.
    ValueError for anything else.  Calls nothing in the library."""
    return _what_codes(what, "rank filter", RANK_WHATS, RANK_BOTHAT, "RANK_COPY (0) .. RANK_BOTHAT (7)")


def rank_radius(radius, codes=()):
    """An integer 0 .. RANK_RADIUS_MAX, and 0 .. RANK_MEDIAN_RADIUS_MAX where `codes` hold RANK_MEDIAN; ValueError for anything else.
    Calls nothing in the library."""
    if RANK_MEDIAN in tuple(codes):
        return _radius(radius, "rank", RANK_MEDIAN_RADIUS_MAX, " for a median")
    return _radius(radius, "rank", RANK_RADIUS_MAX)


def _is_one_what(what):
    return isinstance(what, str) or (len(what) > 0 and not isinstance(what[0], (str, tuple, list)))


def _window_args(family, radii, whats, dsts):
    """(radii, codes per pair) of the pairs of a windowed-plane family, checked.  "local": every radius, then every what.  "rank": every
    what, then every radius against the codes its destination has planes for (the median's limit)."""
    if family == "local":
        radii = [local_radius(r) for r in radii]
        return radii, [local_what_codes(w) for w in whats]
    codes = [rank_what_codes(w) for w in whats]
    return [rank_radius(r, c[:getattr(d, "channels", 3)]) for r, c, d in zip(radii, codes, dsts)], codes


def _window_planes_batch(family, srcs, dsts, radius, what):
    """cvh_<family>_planes_batch: a scalar `radius` and ONE `what` go to every pair, else one per pair."""
    srcs, dsts = _pairs(srcs, dsts)
    n = len(srcs)
    radii = [radius] * n if isinstance(radius, (int, np.integer)) else list(radius)
    whats = [what] * n if _is_one_what(what) else list(what)
    if len(radii) != n or len(whats) != n:
        raise ValueError(f"{n} pairs need {n} radii and {n} codes tuples (or one of each), got {len(radii)} and {len(whats)}")
    radii, codes = _window_args(family, radii, whats, dsts)
    flat = [v for c in codes for v in c]
    call = getattr(lib(), f"cvh_{family}_planes_batch")
    _check(call(_member_array(srcs), _member_array(dsts), n, _array(C.c_int, n, radii), _array(C.c_int, 3 * n, flat)))


def local_planes_batch(srcs, dsts, radius, what):
    """cvh_local_planes_batch: Context.local_planes_to for n pairs (any mix of shapes, channel counts, radii and codes) with one set of
    launches.  A scalar `radius` and ONE `what` (a name or a tuple of codes) go to every pair; else one per pair."""
    _window_planes_batch("local", srcs, dsts, radius, what)


def rank_planes_batch(srcs, dsts, radius, what):
    """cvh_rank_planes_batch: Context.rank_planes_to for n pairs (any mix of shapes, channel counts, radii and codes) with one set of
    launches.  A scalar `radius` and ONE `what` (a name or a tuple of codes) go to every pair; else one per pair.  A median's radius
    limit is checked against the codes a destination has planes for."""
    _window_planes_batch("rank", srcs, dsts, radius, what)


def smooth_what_codes(what):
    """A name -- "blur", "detail" (every plane) -- or 1 to 3 codes -> the three codes cvh_smooth_planes reads; entries a destination has
    no plane for are ignored by the library and filled with SMOOTH_COPY here.  ValueError for anything else.  Calls nothing in the
    library."""
    return _what_codes(what, "smoothing", SMOOTH_WHATS, SMOOTH_DETAIL, "SMOOTH_COPY (0), SMOOTH_BLUR (1), SMOOTH_DETAIL (2)")


def gauss_taps(sigma):
    """cvh_gauss_taps: (radius, taps) of the library's Gaussian of that sigma (0 < sigma <= 21) -- radius = ceil(3 sigma) and radius + 1
    np.uint16 taps whose symmetric sum is 32768.  The C function is the definition; ValueError for what it refuses."""
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)):
        raise ValueError(f"smoothing sigma must be a number in (0, 21], got {sigma!r}")
    taps, radius = (C.c_uint16 * (SMOOTH_RADIUS_MAX + 1))(), C.c_int(0)
    if lib().cvh_gauss_taps(float(sigma), taps, C.byref(radius)) != CVH_OK:
        raise ValueError(f"smoothing sigma must be a finite number in (0, 21], got {sigma!r}")
    return radius.value, np.array(taps[:radius.value + 1], dtype=np.uint16)


def smooth_kernel(kernel):
    """(radius, np.uint16 taps) of a smoothing kernel: a number (float or int) is the Gaussian of that sigma (gauss_taps), an integer SEQUENCE the taps
    t[0 .. R] as given -- 1 to SMOOTH_RADIUS_MAX + 1 of them, each 0 .. 65535, t[0] + 2 (t[1] + .. + t[R]) = 32768.  ValueError for
    anything else.  Only the Gaussian calls the library (a host function that needs no device)."""
    if isinstance(kernel, (int, float, np.integer, np.floating)) and not isinstance(kernel, bool):   # (a bare integer is a sigma, not a tap)
        return gauss_taps(kernel)
    try:
        taps = list(kernel)
    except TypeError:
        taps = None
    if isinstance(kernel, (str, bytes)) or not taps or len(taps) > SMOOTH_RADIUS_MAX + 1 or \
            any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 65535 for v in taps):
        raise ValueError(f"a smoothing kernel is a float sigma or 1 to {SMOOTH_RADIUS_MAX + 1} integer taps 0 .. 65535, got {kernel!r}")
    total = int(taps[0]) + 2 * sum(int(v) for v in taps[1:])
    if total != SMOOTH_TAP_SUM:
        raise ValueError(f"smoothing taps must add up to {SMOOTH_TAP_SUM} over the window (t[0] + 2 sum t[i]), got {total}")
    return len(taps) - 1, np.array(taps, dtype=np.uint16)


def _is_one_kernel(kernel):
    """a float, or a sequence of integers: ONE kernel for every pair (a sequence of floats or of sequences is one per pair)"""
    if isinstance(kernel, (int, float, np.integer, np.floating)) or isinstance(kernel, np.ndarray) and kernel.ndim == 1 and kernel.dtype.kind in "iu":
        return True
    try:
        return len(kernel) > 0 and all(isinstance(v, (int, np.integer)) for v in kernel)
    except TypeError:
        return True                                        # (smooth_kernel says what is wrong with it)


def smooth_planes_batch(srcs, dsts, kernel, what):
    """cvh_smooth_planes_batch: Context.smooth_planes_to for n pairs (any mix of shapes, channel counts, kernels and codes) with one set
    of launches.  ONE `kernel` (a float sigma or a sequence of integer taps) and ONE `what` (a name or a tuple of codes) go to every
    pair; else a list of one per pair."""
    srcs, dsts = _pairs(srcs, dsts)
    n = len(srcs)
    kernels = [kernel] * n if _is_one_kernel(kernel) else list(kernel)
    whats = [what] * n if _is_one_what(what) else list(what)
    if len(kernels) != n or len(whats) != n:
        raise ValueError(f"{n} pairs need {n} kernels and {n} codes tuples (or one of each), got {len(kernels)} and {len(whats)}")
    kernels = [smooth_kernel(k) for k in kernels]
    flat = [v for w in whats for v in smooth_what_codes(w)]
    rows = [_array(C.c_uint16, len(t), [int(v) for v in t]) for _, t in kernels]
    taps = (C.POINTER(C.c_uint16) * n)(*[C.cast(r, C.POINTER(C.c_uint16)) for r in rows])
    _check(lib().cvh_smooth_planes_batch(_member_array(srcs), _member_array(dsts), n, _array(C.c_int, n, [r for r, _ in kernels]), taps,
                                         _array(C.c_int, 3 * n, flat)))


def _coarse_to_fine(pyramids, max_steps, run):
    """The pyramids (each a list of contexts, finest first, all of one depth) advance level by level: run(contexts of a level, max_steps)
    -> [(steps, norm)].  Returns [[(steps, norm)] finest first] per pyramid."""
    pyramids = [list(p) for p in pyramids]
    depth = len(pyramids[0]) if pyramids else 0
    if depth < 1 or any(len(p) != depth for p in pyramids):
        raise ValueError("every pyramid needs the same number of levels, at least one")
    before = [p[0].co_resident for p in pyramids]
    for p in pyramids:   # the levels of a pyramid never stream beside each other
        for ctx in p:
            ctx.set_option("co_resident", 0)
    out = [[None] * depth for _ in pyramids]
    try:
        for k in range(depth - 1):
            restrict_image_batch([p[k] for p in pyramids], [p[k + 1] for p in pyramids])
        for k in range(depth - 1, -1, -1):
            level = [p[k] for p in pyramids]
            if k < depth - 1:
                prolong_levelset_batch([p[k + 1] for p in pyramids], level)
            for ctx, was in zip(level, before):
                ctx.set_option("co_resident", was if k == 0 else 1)
            for i, res in enumerate(run(level, max_steps)):
                out[i][k] = res
            if k:
                for ctx in level:
                    ctx.set_option("co_resident", 0)
    finally:   # (a failed call: the finest level still gets its value back, the helper levels theirs of 0)
        for p, was in zip(pyramids, before):
            p[0].set_option("co_resident", was)
            for ctx in p[1:]:
                ctx.set_option("co_resident", 0)
    return out


def run_coarse_to_fine(levels, max_steps=-1):
    """A coarse-to-fine run of one pyramid.  levels: contexts finest first, shaped as pyramid_shapes gives them; the finest holds the image,
    the coarsest the caller's start (any init_* or set_levelset: planes do not touch a level set, so a start that needs the coarsest planes
    -- threshold, Otsu -- is built after restrict_image_to down the chain, which this call repeats).  Sequence: restrict down the chain,
    Context.run on the coarsest, prolong, run the next level, ... -- max_steps applies per level.  Returns [(steps, norm)], finest first.
    Every level keeps its OWN parameters and options: nothing is rescaled between levels.  While a level runs, the other levels have
    "co_resident" = 0, so each level makes the automatic choices it makes alone on the device; on return the finest has the value it had
    before and the helper levels stay 0."""
    return _coarse_to_fine([levels], max_steps, lambda cs, k: [cs[0].run(k)])[0]


def run_coarse_to_fine_batch(pyramids, max_steps=-1):
    """run_coarse_to_fine over N pyramids of one depth (a list of lists, each finest first): every level of all pyramids is restricted,
    prolonged (one launch each) and advanced with run_batch together.  Returns [[(steps, norm)] finest first] per pyramid."""
    return _coarse_to_fine(pyramids, max_steps, run_batch)


def _segmented(contexts, max_steps, every, run, between=None, after=None):
    """run(contexts, k) -> [(steps, norm)] in segments of `every` iterations; a member whose stop rule fired inside a segment leaves for
    the later ones.  after(ran, live, total) -> live, if given, sees every segment's end -- the indices that ran it, those still
    iterating, the iterations so far -- and returns who goes on; between(contexts still iterating), if given, runs between two
    segments.  every <= 0: one run(contexts, max_steps), and nothing else."""
    if every <= 0 or not contexts:
        return run(contexts, max_steps)
    total, norm = [0] * len(contexts), [0.0] * len(contexts)
    live = list(range(len(contexts)))
    left = max_steps
    while live and left != 0:
        k = every if left < 0 else min(every, left)
        ran = live
        res = run([contexts[i] for i in ran], k)
        for i, (done, nrm) in zip(ran, res):
            total[i] += done
            norm[i] = nrm
        live = [i for i in ran if not contexts[i].sync()[2]]   # (nothing is in flight: sync reports whether the stop rule fired)
        if after is not None:
            live = after(ran, live, total)
        if left > 0:
            left -= k
        if live and left != 0 and between is not None:
            between([contexts[i] for i in live])
    return list(zip(total, norm))


def run_with_reinit(ctx, max_steps=-1, every=0):
    """Context.run in segments of `every` iterations with a reinit between segments; stops as soon as the stop rule fired inside a
    segment (no reinit follows).  max_steps is the total budget (< 0: unlimited).  Returns (total steps, last norm).  every <= 0 is
    exactly ctx.run(max_steps)."""
    return _segmented([ctx], max_steps, every, lambda cs, k: [cs[0].run(k)], between=reinit_batch)[0]


def run_batch_with_reinit(contexts, max_steps=-1, every=0):
    """run_batch in segments of `every` iterations with a reinit_batch between segments.  A member whose stop rule fired inside a
    segment leaves the batch for the later segments (and is not reinitialised again).  Returns [(total steps, last norm)] per context;
    every <= 0 is exactly run_batch(contexts, max_steps)."""
    return _segmented(list(contexts), max_steps, every, run_batch, between=reinit_batch)


def energy_batch(contexts):
    """cvh_energy_batch: Context.energy for n contexts (any mix of shapes and channel counts) with one set of launches and one host
    wait.  Returns [Energy] per context; every value is bit for bit the member's own Context.energy()."""
    contexts, n = _members(contexts)
    out = _array(EnergyTerms, n)
    _check(lib().cvh_energy_batch(_member_array(contexts), n, out))
    return [_energy_of(out[i], contexts[i].channels) for i in range(n)]


def score_batch(contexts, truths, invert=False, tol=2.0, stream=0):
    """cvh_score_mask_device_batch: Context.score for n contexts (any mix of shapes and channel counts) against n truth planes in device
    memory (integer addresses of h * w bytes, non-zero = foreground), with one set of launches and one host wait.  Returns [Score] per
    context; every integer is the member's own Context.score()."""
    contexts, n = _members(contexts)
    out = _array(MaskScore, n)
    _check(lib().cvh_score_mask_device_batch(_member_array(contexts), n, _address_array(truths, n), int(bool(invert)), score_tol2(tol), out, _ptr(stream)))
    return [_score_of(out[i]) for i in range(n)]


def _clean_args(conn, invert, min_area, fill_holes, keep_largest):
    return int(conn), int(bool(invert)), int(min_area), int(fill_holes), int(keep_largest)


def _r2_array(r2, radius, n):
    """one squared radius per member: r2 / radius are one number for all members or one per member"""
    if r2 is not None and radius is not None:
        raise ValueError("give r2 or radius, not both")
    if radius is not None:
        return _array(C.c_uint32, n, _per_member(radius, n, "radius", lambda v: _morph_r2(None, float(v))))
    return _array(C.c_uint32, n, _per_member(0 if r2 is None else r2, n, "r2", lambda v: _morph_r2(v, None)))


def mask_morph_batch(contexts, ptrs, op, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, stream=0):
    """cvh_get_mask_morph_device_batch: Context.mask_morph for n contexts (any mix of shapes and channel counts) into device memory (ptrs:
    one integer address of h * w bytes per context), one set of launches for all; r2 / radius are one number or one per member, op is
    shared.  Work enqueued on `stream` afterwards sees the masks.  Does not block the host."""
    contexts, n = _members(contexts)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (morph_code(op), _r2_array(r2, radius, n))
    _check(lib().cvh_get_mask_morph_device_batch(_member_array(contexts), n, _address_array(ptrs, n), *args, _ptr(stream)))


def morph_levelset_batch(contexts, op, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, inside=1.0,
                         outside=-1.0):
    """cvh_morph_levelset_batch: Context.morph_levelset for n contexts with one set of launches; r2 / radius as in mask_morph_batch."""
    contexts, n = _members(contexts)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (morph_code(op), _r2_array(r2, radius, n))
    _check(lib().cvh_morph_levelset_batch(_member_array(contexts), n, *args, float(inside), float(outside)))


def split_geometry():
    """cvh_split_geometry: (tile_rows, tile_cols, group) -- the tile of the growth's sweeps and the sweeps enqueued per host wait."""
    tr, tc, g = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().cvh_split_geometry(C.byref(tr), C.byref(tc), C.byref(g))
    return tr.value, tc.value, g.value


def split_batch(contexts, ptrs=None, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, stream=0):
    """cvh_split_batch: Context.split for n contexts (any mix of shapes and channel counts) with one set of launches.  ptrs: one integer
    device address of h * w int32 labels per context (0 = no label plane for that member), or None; r2 / radius are one number or one per
    member.  Returns [K] per context."""
    contexts, n = _members(contexts)
    counts = _array(C.c_int, n)
    addr = None if ptrs is None else _address_array(ptrs, n)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (_r2_array(r2, radius, n),)
    _check(lib().cvh_split_batch(_member_array(contexts), n, *args, addr, counts, _ptr(stream)))
    return [counts[i] for i in range(n)]


def split_levelset_batch(contexts, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, inside=1.0,
                         outside=-1.0):
    """cvh_split_levelset_batch: Context.split_levelset for n contexts with one set of launches; r2 / radius as in split_batch."""
    contexts, n = _members(contexts)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (_r2_array(r2, radius, n),)
    _check(lib().cvh_split_levelset_batch(_member_array(contexts), n, *args, float(inside), float(outside)))


def init_mask_batch(contexts, ptrs, inside=1.0, outside=-1.0, stream=0):
    """cvh_init_mask_device_batch: Context.init_mask for n contexts from byte masks in device memory (ptrs: one integer address of h * w
    bytes per context, read behind what `stream` holds), one launch for all."""
    contexts, n = _members(contexts)
    _check(lib().cvh_init_mask_device_batch(_member_array(contexts), n, _address_array(ptrs, n), float(inside), float(outside),
                                                _ptr(stream)))


def measure_batch(contexts, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, cap=None, stream=0):
    """cvh_measure_batch: Context.measure for n contexts (any mix of shapes and channel counts) with one set of launches.  cap: None
    (all rows, at the price of a first call for the counts), one number for every member or one per member.  Returns [(K, table)] per
    context; every row is bit for bit the member's own Context.measure()."""
    contexts, n = _members(contexts)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest)
    counts = _array(C.c_int, n)

    def call(tables, caps):
        _check(lib().cvh_measure_batch(_member_array(contexts), n, *args, tables, caps, counts, _ptr(stream)))
        return counts[:n]
    caps = _caps_batch(call, cap, n, "cap")
    if cap is None and not any(c > 0 for c in caps):   # (counted, and nothing to fetch: no second call)
        return [(c, np.zeros(0, dtype=REGION_DTYPE)) for c in caps]
    rows = _rows_batch(call, REGION_DTYPE, caps, C.c_int)
    return list(zip(counts[:n], rows))


def overlaps_batch(contexts, others, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, cap=None, stream=0):
    """cvh_overlaps_device_batch: Context.overlaps for n contexts (any mix of shapes and channel counts) against n int32 label planes in
    device memory (integer addresses of h * w int32), with one set of launches.  cap: None (all rows, at the price of a first call for
    the counts), one number for every member or one per member.  Returns [(rows, K)] per context; every row is byte for byte the
    member's own Context.overlaps()."""
    contexts, n = _members(contexts)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest)
    pairs, counts = _array(C.c_long, n), _array(C.c_int, n)
    ptrs = _address_array(others, n)

    def call(tables, caps):
        _check(lib().cvh_overlaps_device_batch(_member_array(contexts), n, *args, ptrs, tables, caps, pairs, counts, _ptr(stream)))
        return pairs[:n]
    rows = _rows_batch(call, OVERLAP_DTYPE, _caps_batch(call, cap, n, "cap"), C.c_long)   # (the second call is always made)
    return list(zip(rows, counts[:n]))


def _threshold(threshold):
    """(num, den) of an IoU threshold: a pair of integers as it is, a number as the nearest multiple of 1/1000"""
    if np.ndim(threshold):
        num, den = (int(v) for v in threshold)
        return num, den
    return int(round(float(threshold) * 1000)), 1000


def match_overlaps(rows, threshold=(1, 2)):
    """cvh_match_overlaps on a table of Context.overlaps (OVERLAP_DTYPE, all P rows): the components (a != 0) against the objects of
    the other plane (b != 0) at the IoU threshold num / den (a pair of integers, or a number taken in thousandths; 1/2 <= t <= 1,
    strictly-above).  Returns (score, match_of_a, ious): score an ObjectScore at the threshold, with tp at 10/20 .. 19/20 for mean_ap;
    match_of_a an int32 array whose entry a - 1 is the b that component a matched, or 0; ious a list of (a, b, num, den) per matched
    pair, the exact IoU count / (area_a + area_b - count) in Python integers.  Host arithmetic, no device."""
    rows = np.ascontiguousarray(rows, dtype=OVERLAP_DTYPE).reshape(-1)
    num, den = _threshold(threshold)
    k = int(rows["a"].max()) if rows.size else 0
    match_of_a = np.zeros(max(k, 0), np.int32)
    L = lib()

    def at(nu, de, out_match):
        m = Match()
        rc = L.cvh_match_overlaps(rows.ctypes.data if rows.size else None, rows.size, nu, de,
                                  out_match.ctypes.data if out_match is not None and out_match.size else None, max(k, 0), C.byref(m))
        if rc != CVH_OK:
            raise CvhError(rc, f"cvh_match_overlaps: {rows.size} rows at {nu}/{de}")
        return m
    m = at(num, den, match_of_a)
    tp_at = tuple(int(at(t, 20, None).tp) for t in range(10, 20))
    area_a, area_b = {}, {}
    for a, b, c in zip(rows["a"].tolist(), rows["b"].tolist(), rows["count"].tolist()):
        area_a[a] = area_a.get(a, 0) + c
        area_b[b] = area_b.get(b, 0) + c
    ious = [(a, b, c, area_a[a] + area_b[b] - c) for a, b, c in zip(rows["a"].tolist(), rows["b"].tolist(), rows["count"].tolist())
            if a != 0 and b != 0 and match_of_a[a - 1] == b]
    return ObjectScore(int(m.objects_a), int(m.objects_b), int(m.tp), int(m.fp), int(m.fn), tp_at), match_of_a, ious


def _contours_batch(fn, args, contexts, d_points, point_caps, loop_caps, stream):
    """cvh_contours_device_batch or cvh_contours_subpixel_device_batch (fn) with the options args: what contours_batch documents"""
    contexts, n = _members(contexts)
    nloops, npoints = _array(C.c_long, n), _array(C.c_long, n)
    points = None, None   # (the point arrays and their caps: a first call for the counts comes before they are looked at)

    def call(tables, caps):
        _check(fn(_member_array(contexts), n, *args, tables, caps, *points, nloops, npoints, _ptr(stream)))
        return nloops[:n]
    loop_caps = _caps_batch(call, loop_caps, n, "loop_caps")
    if d_points is not None:
        d_points, point_caps = list(d_points), [int(c) for c in point_caps]
        if len(d_points) != n or len(point_caps) != n:
            raise ValueError(f"{n} contexts but {len(d_points)} point arrays and {len(point_caps)} caps")
        points = _address_array(d_points, n), _array(C.c_long, n, point_caps)
    rows = _rows_batch(call, CONTOUR_LOOP_DTYPE, loop_caps, C.c_long)   # (the second call is always made)
    return list(zip(nloops[:n], npoints[:n], rows))


def contours_batch(contexts, d_points=None, point_caps=None, conn=8, invert=False, min_area=0, fill_holes=0, keep_largest=False, simplify=True,
                   loop_caps=None, stream=0):
    """cvh_contours_device_batch: Context.contours for n contexts (any mix of shapes and channel counts) with one set of launches.
    d_points: None (no points), or per member the integer address of device memory for point_caps[i] points (two int32 each; 0: none
    for that member).  loop_caps: None (every row, at the price of a first call for the counts) or one number per member.  Returns
    [(nloops, npoints, loops)] per context, loops a structured array (CONTOUR_LOOP_DTYPE) of the first min(nloops, cap) rows; rows and
    points are bit for bit the member's own Context.contours()."""
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (int(bool(simplify)),)
    return _contours_batch(lib().cvh_contours_device_batch, args, contexts, d_points, point_caps, loop_caps, stream)


def contours_subpixel_batch(contexts, d_points=None, point_caps=None, conn=8, invert=False, min_area=0, fill_holes=0, keep_largest=False,
                            loop_caps=None, stream=0):
    """cvh_contours_subpixel_device_batch: Context.contours_subpixel for n contexts with one set of launches -- contours_batch without
    simplify; a point is two float64 (16 bytes, the address 8-byte aligned).  Rows and points are bit for bit the member's own
    Context.contours_subpixel()."""
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest)
    return _contours_batch(lib().cvh_contours_subpixel_device_batch, args, contexts, d_points, point_caps, loop_caps, stream)


def contour_subpixel_measures(loops, points):
    """cvh_contour_subpixel_measure for every loop of Context.contours_subpixel(): (area, length), two float64 arrays with one entry per
    loop -- the polygon's signed area (positive for an outer boundary, negative for a hole) and its perimeter, each a sequential FP64
    sum over the loop's points in order.  Host arithmetic, no device."""
    loops = np.ascontiguousarray(loops, dtype=CONTOUR_LOOP_DTYPE).reshape(-1)
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    area, length = np.zeros(loops.size), np.zeros(loops.size)
    spare = np.zeros(2)   # (an address for a loop without points)
    L = lib()
    for k in range(loops.size):
        first, n = int(loops["offset"][k]), int(loops["points"][k])
        if first + n > points.shape[0]:
            raise ValueError(f"loop {k}: points {first} .. {first + n - 1} of {points.shape[0]}")
        a, ln = C.c_double(0.0), C.c_double(0.0)
        rc = L.cvh_contour_subpixel_measure(points.ctypes.data + 16 * first if n else spare.ctypes.data, n, C.byref(a), C.byref(ln))
        if rc != CVH_OK:
            raise CvhError(rc, f"cvh_contour_subpixel_measure: loop {k}, {n} points")
        area[k], length[k] = a.value, ln.value
    return area, length


def region_shapes(table, channels):
    """cvh_region_shape_of for every row of a measure table (REGION_DTYPE): a structured array (REGION_SHAPE_DTYPE) of centroid, central
    moments, orientation, the axes of the ellipse with the same moments, and mean and variance per channel.  Host arithmetic, no device."""
    table = np.ascontiguousarray(table, dtype=REGION_DTYPE).reshape(-1)
    out = np.zeros(table.size, dtype=REGION_SHAPE_DTYPE)
    L = lib()
    for i in range(table.size):
        rc = L.cvh_region_shape_of(table.ctypes.data + i * REGION_DTYPE.itemsize, int(channels), out.ctypes.data + i * REGION_SHAPE_DTYPE.itemsize)
        if rc != CVH_OK:
            raise CvhError(rc, f"cvh_region_shape_of: row {i} (area {int(table['area'][i])}), channels {channels}")
    return out


def _monitor_args(max_steps, every, rel_plateau):
    for name, v in (("max_steps", max_steps), ("every", every)):
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError(f"{name} must be an int, got {v!r}")
    if rel_plateau is None:
        return
    if isinstance(rel_plateau, bool) or not isinstance(rel_plateau, (int, float)) or not math.isfinite(rel_plateau) or rel_plateau < 0:
        raise ValueError(f"rel_plateau must be None or a finite number >= 0, got {rel_plateau!r}")
    if every <= 0:
        raise ValueError("rel_plateau compares the energies of two segments: it needs every > 0")


def _monitored(contexts, max_steps, every, rel_plateau, run):
    """_segmented with one energy_batch behind every segment, over the members that ran it.  Returns [(steps, norm, series)]."""
    _monitor_args(max_steps, every, rel_plateau)
    series = [[] for _ in contexts]

    def after(ran, live, total):
        plateaued = set()
        for i, e in zip(ran, energy_batch([contexts[j] for j in ran])):
            prev = series[i][-1][1].total if series[i] else None
            series[i].append((total[i], e))
            if rel_plateau is not None and prev is not None and abs(prev - e.total) <= rel_plateau * abs(prev):
                plateaued.add(i)
        return [i for i in live if i not in plateaued]

    if every <= 0:
        res = run(contexts, max_steps)
        after(list(range(len(contexts))), [], [r[0] for r in res])
    else:
        res = _segmented(contexts, max_steps, every, run, after=after)
    return [(done, nrm, ser) for (done, nrm), ser in zip(res, series)]


def multiphase_geometry(h, w):
    """cvh_multiphase_geometry: (columns per wave, rows per strip, items) of the fixed partition the four-phase sums are taken over;
    pure host arithmetic (rows and items are 0 for a plane the calls refuse)."""
    cols, rows, items = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().cvh_multiphase_geometry(int(h), int(w), C.byref(cols), C.byref(rows), C.byref(items))
    return cols.value, rows.value, items.value


def _trace_rows_wanted(max_steps, trace):
    want = 0 if trace is False or trace is None else (int(max_steps) if trace is True else int(trace))
    if want < 0:
        raise ValueError("trace=True needs max_steps >= 0 (or pass the number of rows)")
    return want


def _trace_out(want, trace, tail):
    """the buffer a march call writes its trace into, max(want, 1) rows of shape `tail` -- or None where no trace is asked for"""
    return np.zeros((max(want, 1),) + tail, dtype=np.float64) if want or trace is True else None


def _trace_of(out, rows):
    return None if out is None else out[:rows].copy()


def _march_run_batch(what, fn, lists, leading, tail, norms_per, max_steps, trace):
    """What the three *_run_batch wrappers share.  lists: the member lists (two: the halves of n pairs); leading(n): the arguments the
    call takes between n and max_steps, checked before any handle is read; tail(member of the first list): the shape of one of its
    trace rows; norms_per: the norms the call reports per member.  Returns [(steps_done, norm or tuple of norms, trace)]."""
    lists = [list(m) for m in lists]
    n = len(lists[0])
    if n == 0:
        raise ValueError(f"{what}: no {'pairs' if len(lists) > 1 else 'members'}")
    lead = leading(n)
    want = _trace_rows_wanted(max_steps, trace)
    done, rows, norms = _array(C.c_int, n), _array(C.c_int, n), _array(C.c_double, norms_per * n)
    outs = [_trace_out(want, trace, tail(m)) for m in lists[0]]
    traces = None if outs[0] is None else _array(C.c_void_p, n, [o.ctypes.data for o in outs])
    _check(fn(*[_member_array(m) for m in lists], n, *lead, int(max_steps), done, norms, traces, want, rows))
    norm_of = (lambda i: norms[i]) if norms_per == 1 else (lambda i: tuple(norms[norms_per * i:norms_per * (i + 1)]))
    return [(done[i], norm_of(i), _trace_of(outs[i], rows[i])) for i in range(n)]


def multiphase_run(a, b, max_steps=-1, trace=False):
    """cvh_multiphase_run ("Four phases" in include/chanvese_hip.h): contexts a and b hold phi1 and phi2 of a Vese-Chan pair and are
    iterated together until max_steps iterations are done (negative: no bound) or the pair stops.  Returns (steps_done, (norm1, norm2),
    trace): trace is None, or with trace=True (all rows; needs max_steps >= 0) or trace=<rows> an array of one row of 4 C + 2 doubles
    per iteration -- the means c11, c10, c01, c00 it used and its two norms.  Both contexts are left as set_levelset of the new level
    sets leaves them."""
    want = _trace_rows_wanted(max_steps, trace)
    done, rows, norms = C.c_int(0), C.c_int(0), (C.c_double * 2)()
    out = _trace_out(want, trace, (4 * a.channels + 2,))
    _check(lib().cvh_multiphase_run(a._h, b._h, int(max_steps), C.byref(done), norms, None if out is None else _dp(out), want, C.byref(rows)))
    return done.value, (norms[0], norms[1]), _trace_of(out, rows.value)


def multiphase_run_batch(pairs, max_steps=-1, trace=False):
    """cvh_multiphase_run_batch: multiphase_run for every pair (a, b) of `pairs` at once -- per iteration one step launch and one
    finalise launch for all pairs of a (channel count, math mode) class.  Every pair iterates and stops on its own and is bit for bit
    what multiphase_run gives for it alone.  Returns a list of (steps_done, (norm1, norm2), trace), one per pair; trace as there."""
    pairs = [tuple(p) for p in pairs]
    if any(len(p) != 2 for p in pairs):
        raise ValueError("multiphase_run_batch: every member is a pair (a, b) of contexts")
    return _march_run_batch("multiphase_run_batch", lib().cvh_multiphase_run_batch, ([a for a, _ in pairs], [b for _, b in pairs]), lambda n: (),
                            lambda a: (4 * a.channels + 2,), 2, max_steps, trace)


def multiphase_means(a, b):
    """cvh_multiphase_means: the means of the current pair as an array of (4, C), rows c11, c10, c01, c00.  Only reads."""
    c = np.zeros((4, a.channels), dtype=np.float64)
    _check(lib().cvh_multiphase_means(a._h, b._h, _dp(c)))
    return c


def localized_geometry(h, w, radius):
    """cvh_localized_geometry: (columns per wave, rows per item, items, rows per strip) -- the fixed partition the norm of the localised
    run is summed over (a function of h and w alone) and the rows one wave marches down at this radius; pure host arithmetic (rows and
    items are 0 for a plane or radius the calls refuse)."""
    cols, rows, items, strip = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    lib().cvh_localized_geometry(int(h), int(w), int(radius), C.byref(cols), C.byref(rows), C.byref(items), C.byref(strip))
    return cols.value, rows.value, items.value, strip.value


def localized_run(ctx, radius, max_steps=-1, trace=False):
    """cvh_localized_run ("Localised regions" in include/chanvese_hip.h): localised Chan-Vese with the region means taken over the
    (2 radius + 1)^2 window of every pixel, until max_steps iterations are done (negative: no bound) or the stop rule fires.  Returns
    (steps_done, norm, trace): trace is None, or with trace=True (all rows; needs max_steps >= 0) or trace=<rows> an array of the
    iterations' ||d||.  The context is left as set_levelset of the new level set leaves it.  The local force is small: start near the
    object and raise mu."""
    want = _trace_rows_wanted(max_steps, trace)
    done, rows, norm = C.c_int(0), C.c_int(0), C.c_double(0.0)
    out = _trace_out(want, trace, ())
    ctx._chk(lib().cvh_localized_run(ctx._h, int(radius), int(max_steps), C.byref(done), C.byref(norm), None if out is None else _dp(out), want,
                                     C.byref(rows)))
    return done.value, norm.value, _trace_of(out, rows.value)


def localized_run_batch(contexts, radius, max_steps=-1, trace=False):
    """cvh_localized_run_batch: localized_run for every context at once -- per iteration one row-pass, one step and one finalise launch
    for all members of a (channel count, math mode) class.  radius is an int (the same for every member) or a sequence of one value per
    member.  Every member iterates and stops on its own and is bit for bit what localized_run gives for it alone.  Returns a list of
    (steps_done, norm, trace), one per member; trace as there."""
    return _march_run_batch("localized_run_batch", lib().cvh_localized_run_batch, (contexts,),
                            lambda n: (_array(C.c_int, n, _per_member(radius, n, "radius", int)),), lambda c: (), 1, max_steps, trace)


def geodesic_geometry(h, w):
    """cvh_geodesic_geometry: (columns per wave, rows per strip, items) of the fixed partition the edge-weighted run's sums are taken
    over -- the four-phase partition; pure host arithmetic (rows and items are 0 for a plane the calls refuse)."""
    cols, rows, items = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().cvh_geodesic_geometry(int(h), int(w), C.byref(cols), C.byref(rows), C.byref(items))
    return cols.value, rows.value, items.value


def edge_map_batch(dsts, srcs, K):
    """cvh_edge_map_batch: Context.edge_map_from for n pairs (any mix of shapes and channel counts) in one launch.  K is one value for
    every pair or one per pair."""
    dsts, srcs = list(dsts), list(srcs)
    n = len(dsts)
    if n == 0 or len(srcs) != n:
        raise ValueError(f"edge_map_batch: {n} destinations, {len(srcs)} sources")
    ks = _array(C.c_double, n, _per_member(K, n, "K", float))
    _check(lib().cvh_edge_map_batch(_member_array(dsts), _member_array(srcs), n, ks))


def geodesic_run(ctx, max_steps=-1, trace=False):
    """cvh_geodesic_run ("Edge-weighted length" in include/chanvese_hip.h): Chan-Vese with the length term weighted by the context's
    edge plane, until max_steps iterations are done (negative: no bound) or the stop rule fires.  Returns (steps_done, norm, trace):
    trace is None, or with trace=True (all rows; needs max_steps >= 0) or trace=<rows> an array of one row of 2 C + 1 doubles per
    iteration -- the means c1, c2 it used and its norm.  The context is left as set_levelset of the new level set leaves it."""
    want = _trace_rows_wanted(max_steps, trace)
    done, rows, norm = C.c_int(0), C.c_int(0), C.c_double(0.0)
    out = _trace_out(want, trace, (2 * ctx.channels + 1,))
    ctx._chk(lib().cvh_geodesic_run(ctx._h, int(max_steps), C.byref(done), C.byref(norm), None if out is None else _dp(out), want, C.byref(rows)))
    return done.value, norm.value, _trace_of(out, rows.value)


def geodesic_run_batch(contexts, max_steps=-1, trace=False):
    """cvh_geodesic_run_batch: geodesic_run for every context at once -- per iteration one step and one finalise launch for all members
    of a (channel count, math mode) class.  Every member iterates and stops on its own and is bit for bit what geodesic_run gives for
    it alone.  Returns a list of (steps_done, norm, trace), one per member; trace as there."""
    return _march_run_batch("geodesic_run_batch", lib().cvh_geodesic_run_batch, (contexts,), lambda n: (), lambda c: (2 * c.channels + 1,), 1,
                            max_steps, trace)


def convex_geometry(h, w):
    """cvh_convex_geometry: (columns per wave, rows per strip, items) of the fixed partition the convex run's sums are taken over -- the
    four-phase partition; pure host arithmetic (rows and items are 0 for a plane the calls refuse)."""
    cols, rows, items = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().cvh_convex_geometry(int(h), int(w), C.byref(cols), C.byref(rows), C.byref(items))
    return cols.value, rows.value, items.value


def make_convex_params(tau=0.25, sigma=None, stop_rms=0.0, means_every=1, use_edge=False, resume=False):
    """struct cvh_convex_params ("Convex relaxation" in include/chanvese_hip.h); sigma defaults to 1 / (8 tau), the largest the
    step-size bound 8 tau sigma <= 1 allows."""
    tau = float(tau)
    return ConvexParams(tau, 1.0 / (8.0 * tau) if sigma is None else float(sigma), float(stop_rms), int(means_every), int(bool(use_edge)),
                        int(bool(resume)))


def _convex_params(params):
    return params if isinstance(params, ConvexParams) else make_convex_params(**dict(params or {}))


def convex_run(ctx, max_steps=-1, params=None, trace=False):
    """cvh_convex_run ("Convex relaxation" in include/chanvese_hip.h): the primal-dual iteration of the relaxed two-phase model from the
    mask of the context's level set (or, with resume, from the stored relaxation state), until max_steps iterations are done
    (negative: no bound) or the stop rule of `params` (a ConvexParams, or a dict of make_convex_params' arguments) fires.  Returns
    (steps_done, norm, trace): trace is None, or with trace=True (all rows; needs max_steps >= 0) or trace=<rows> an array of one row of
    2 C + 1 doubles per iteration -- the means c1, c2 it used and its norm.  The context's level set becomes v - 0.5."""
    p = _convex_params(params)
    want = _trace_rows_wanted(max_steps, trace)
    done, rows, norm = C.c_int(0), C.c_int(0), C.c_double(0.0)
    out = _trace_out(want, trace, (2 * ctx.channels + 1,))
    ctx._chk(lib().cvh_convex_run(ctx._h, int(max_steps), C.byref(p), C.byref(done), C.byref(norm), None if out is None else _dp(out), want,
                                  C.byref(rows)))
    return done.value, norm.value, _trace_of(out, rows.value)


def convex_run_batch(contexts, max_steps=-1, params=None, trace=False):
    """cvh_convex_run_batch: convex_run for every context at once -- per iteration one step and one finalise launch for all members of a
    (channel count, math mode) class.  params is one set for every member or a sequence of one per member.  Every member iterates and
    stops on its own and is bit for bit what convex_run gives for it alone.  Returns a list of (steps_done, norm, trace), one per member."""
    contexts = list(contexts)
    n = len(contexts)
    each = [_convex_params(q) for q in params] if isinstance(params, (list, tuple)) else [_convex_params(params)] * n
    if len(each) != n:
        raise ValueError(f"convex_run_batch: {len(each)} parameter sets for {n} members")
    table = _array(ConvexParams, n, each)
    fn = lambda members, count, steps, *rest: lib().cvh_convex_run_batch(members, count, steps, table, *rest)
    return _march_run_batch("convex_run_batch", fn, (contexts,), lambda k: (), lambda c: (2 * c.channels + 1,), 1, max_steps, trace)


def run_monitored(ctx, max_steps=-1, every=16, rel_plateau=None):
    """Context.run in segments of `every` iterations with the energy (Context.energy) taken after each segment.  Returns (total steps,
    last norm, [(steps so far, Energy)]).  max_steps is the total budget (< 0: unlimited); the run ends when the stop rule fired inside
    a segment or the budget is spent, and with rel_plateau = x also as soon as a segment's energy E satisfies |E_prev - E| <= x |E_prev|
    against the segment before it (the first segment has none).  The stop rule itself is not changed.  every <= 0 is exactly
    ctx.run(max_steps) plus one final energy."""
    return _monitored([ctx], max_steps, every, rel_plateau, lambda cs, k: [cs[0].run(k)])[0]


def run_batch_monitored(contexts, max_steps=-1, every=16, rel_plateau=None):
    """run_monitored over run_batch, with one energy_batch per segment.  A member whose stop rule fired or whose energy plateaued leaves
    the batch for the later segments.  Returns [(total steps, last norm, [(steps so far, Energy)])] per context; every <= 0 is exactly
    run_batch(contexts, max_steps) plus one energy_batch."""
    return _monitored(list(contexts), max_steps, every, rel_plateau, run_batch)


class Context:
    """One image on one GPU: thin RAII wrapper over cvh_context."""

    def __init__(self, h, w, channels=1, params=None, device=0):
        self._L = lib()
        self._h = C.c_void_p(None)
        self.h, self.w, self.channels = h, w, channels
        self.co_resident = 1   # the option's value, kept for the pyramid drivers (the library has no getter)
        p = params if params is not None else make_params()
        rc = self._L.cvh_create(C.byref(self._h), h, w, channels, C.byref(p), device)
        if rc != CVH_OK:
            self._h = C.c_void_p(None)
            _check(rc)

    def _chk(self, rc):
        if rc != CVH_OK:
            raise CvhError(rc, self._L.cvh_last_error(self._h).decode())

    def close(self):
        if self._h:
            self._L.cvh_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_params(self, params):
        self._chk(self._L.cvh_set_params(self._h, C.byref(params)))

    def set_option(self, key, value):
        self._chk(self._L.cvh_set_option(self._h, key.encode(), int(value)))
        if key == "co_resident":
            self.co_resident = int(value != 0)

    def _plane_array(self, planes):
        assert len(planes) == self.channels
        keep = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
        for p in keep:
            assert p.shape == (self.h, self.w)
        arr = (C.POINTER(C.c_uint8) * len(keep))(*[_u8p(p) for p in keep])
        return keep, arr

    def set_image(self, planes):
        keep, arr = self._plane_array(planes)
        self._chk(self._L.cvh_set_image(self._h, arr))

    # device-memory forms: `ptr` is an integer device address, `stream` a HIP stream handle as integer (0 = the default stream)
    def set_image_device(self, ptr, layout=LAYOUT_PLANAR, stream=0):
        self._chk(self._L.cvh_set_image_device(self._h, _ptr(ptr), int(layout), _ptr(stream)))

    def get_image_device(self, ptr, layout=LAYOUT_PLANAR, stream=0):
        self._chk(self._L.cvh_get_image_device(self._h, _ptr(ptr), int(layout), _ptr(stream)))

    def set_levelset_device(self, ptr, bits=64, stream=0):
        self._chk(self._L.cvh_set_levelset_device(self._h, _ptr(ptr), int(bits), _ptr(stream)))

    def get_levelset_device(self, ptr, bits=64, stream=0):
        self._chk(self._L.cvh_get_levelset_device(self._h, _ptr(ptr), int(bits), _ptr(stream)))

    def get_mask_device(self, ptr, invert=False, stream=0):
        self._chk(self._L.cvh_get_mask_device(self._h, _ptr(ptr), int(bool(invert)), _ptr(stream)))

    def get_image(self):
        outs = [np.empty((self.h, self.w), dtype=np.uint8) for _ in range(self.channels)]
        arr = (C.POINTER(C.c_uint8) * len(outs))(*[_u8p(p) for p in outs])
        self._chk(self._L.cvh_get_image(self._h, arr))
        return outs

    def set_levelset(self, u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        assert u.shape == (self.h, self.w)
        self._chk(self._L.cvh_set_levelset(self._h, _dp(u)))

    def init_checkerboard(self):
        self._chk(self._L.cvh_init_checkerboard(self._h))

    def histogram(self, cap=None):
        """cvh_histogram: hist[v] = the number of pixels whose grey value g = sum of the planes is v, v = 0 .. 255 C, counted on the device;
        cap (None: all) copies only the first bins.  Returns a uint32 array."""
        bins = C.c_int(0)
        out = np.zeros(255 * self.channels + 1 if cap is None else max(int(cap), 0), dtype=np.uint32)
        self._chk(self._L.cvh_histogram(self._h, out.ctypes.data if out.size else None, int(out.size if cap is None else cap), C.byref(bins)))
        return out[:min(out.size, bins.value)]

    def otsu_threshold(self):
        """cvh_otsu_threshold: Otsu's threshold of the grey values (the header's integer definition)."""
        t = C.c_int(-1)
        self._chk(self._L.cvh_otsu_threshold(self._h, C.byref(t)))
        return t.value

    def init_threshold(self, t, inside=1.0, outside=-1.0):
        """cvh_init_threshold: u = inside where the grey value exceeds t, outside elsewhere, on the device; begins a new run."""
        self._chk(self._L.cvh_init_threshold(self._h, int(t), float(inside), float(outside)))

    def init_otsu(self, inside=1.0, outside=-1.0):
        """cvh_init_otsu: init_threshold at Otsu's threshold, which it returns."""
        t = C.c_int(-1)
        self._chk(self._L.cvh_init_otsu(self._h, C.byref(t), float(inside), float(outside)))
        return t.value

    def init_rect(self, x, y, w, h, inside=1.0, outside=0.0):
        """cvh_init_rect: u = inside on the rectangle's pixels (clipped to the plane), outside elsewhere, on the device."""
        self._chk(self._L.cvh_init_rect(self._h, int(x), int(y), int(w), int(h), float(inside), float(outside)))

    def init_disk(self, cx, cy, r, inside=1.0, outside=0.0):
        """cvh_init_disk: u = inside on the filled disk (col - cx)^2 + (row - cy)^2 <= r^2, outside elsewhere, on the device."""
        self._chk(self._L.cvh_init_disk(self._h, int(cx), int(cy), int(r), float(inside), float(outside)))

    def restrict_image_to(self, coarse):
        """cvh_restrict_image: the planes of this context, averaged 2 x 2 in integers, become the image of `coarse` (a context of
        ((h + 1) // 2, (w + 1) // 2) and the same channel count), exactly as its set_image of those bytes; this context is only read."""
        _check(self._L.cvh_restrict_image(self._h, coarse._h))

    def prolong_levelset_to(self, fine):
        """cvh_prolong_levelset: the level set of this context, replicated 2 x 2 bit for bit, becomes the level set of `fine`, exactly
        as its set_levelset of those doubles (a new run begins there); this context is only read."""
        _check(self._L.cvh_prolong_levelset(self._h, fine._h))

    def convert_colour(self, space, order="bgr", inverse=False):
        """cvh_convert_colour: the three planes, read as (B, G, R) or (R, G, B) by `order`, become (Y, Cr, Cb) ("ycrcb") or (Y, U, V)
        ("yuv") in place on the device -- or, with inverse, back --, exactly as set_image of the converted bytes (the header's integer
        definition).  The library does not remember which space the planes are in."""
        space, order = colour_space_code(space), order_code(order)
        _check(self._L.cvh_convert_colour(self._h, space, order, int(bool(inverse))))

    def luma_to(self, dst, order="bgr"):
        """cvh_luma_image: the Y of this three-channel context becomes the image of `dst` (a one-channel context of the same shape),
        exactly as its set_image of that plane; this context is only read."""
        order = order_code(order)
        _check(self._L.cvh_luma_image(self._h, dst._h, order))

    def _window_planes_to(self, family, dst, radius, what):
        radii, codes = _window_args(family, [radius], [what], [dst])   # (checked before the library is reached)
        _check(getattr(self._L, f"cvh_{family}_planes")(self._h, dst._h, radii[0], (C.c_int * 3)(*codes[0])))

    def local_planes_to(self, dst, radius, what):
        """cvh_local_planes: plane k of `dst` (another context of the same shape, 1 or 3 channels) becomes the copy, the local mean or
        the local deviation over the (2 radius + 1)^2 window of plane min(k, channels - 1) of this context, which is only read.  `what`
        is "mean", "dev", "stack" or a tuple of LOCAL_COPY / LOCAL_MEAN / LOCAL_DEV; `dst` is left as set_image of those planes."""
        self._window_planes_to("local", dst, radius, what)

    def rank_planes_to(self, dst, radius, what):
        """cvh_rank_planes: plane k of `dst` (another context of the same shape, 1 or 3 channels) becomes the copy, minimum, maximum,
        median, opening, closing, white or black top-hat over the (2 radius + 1)^2 window of plane min(k, channels - 1) of this context,
        which is only read.  `what` is "min", "max", "median", "open", "close", "tophat", "bothat" or a tuple of RANK_* codes; `dst` is
        left as set_image of those planes."""
        self._window_planes_to("rank", dst, radius, what)

    def smooth_planes_to(self, dst, kernel, what):
        """cvh_smooth_planes: plane k of `dst` (another context of the same shape, 1 or 3 channels) becomes the copy, the blur or the
        detail (128 + p - blur, clamped) of plane min(k, channels - 1) of this context, which is only read, under a symmetric separable
        kernel with a replicated border.  `kernel` is a float (the Gaussian of that sigma, gauss_taps) or a sequence of integer taps;
        `what` is "blur", "detail" or a tuple of SMOOTH_COPY / SMOOTH_BLUR / SMOOTH_DETAIL; `dst` is left as set_image of those planes."""
        codes = smooth_what_codes(what)                        # (checked before the library is reached)
        radius, taps = smooth_kernel(kernel)
        row = (C.c_uint16 * len(taps))(*[int(v) for v in taps])
        _check(self._L.cvh_smooth_planes(self._h, dst._h, radius, row, (C.c_int * 3)(*codes)))

    def reinit(self):
        """cvh_reinit: the level set becomes the exact signed distance to the pixel-edge front of its own mask, on the device.
        Returns whether it changed (False: the mask is uniform, nothing about the context moved)."""
        changed = C.c_int(0)
        self._chk(self._L.cvh_reinit(self._h, C.byref(changed)))
        return bool(changed.value)

    def get_levelset(self):
        u = np.empty((self.h, self.w), dtype=np.float64)
        self._chk(self._L.cvh_get_levelset(self._h, _dp(u)))
        return u

    def run(self, max_steps=-1):
        """Returns (steps_done, last_norm)."""
        done, nrm = C.c_int(0), C.c_double(0.0)
        self._chk(self._L.cvh_run(self._h, int(max_steps), C.byref(done), C.byref(nrm)))
        return done.value, nrm.value

    def enqueue_steps(self, n):
        self._chk(self._L.cvh_enqueue_steps(self._h, int(n)))

    def warm(self, n):
        """One-off host work of an upcoming enqueue_steps(n) (graph build), outside any timed region."""
        self._chk(self._L.cvh_warm(self._h, int(n)))

    def sync(self):
        """Returns (steps_done_total, last_norm, stopped)."""
        done, nrm, stopped = C.c_int(0), C.c_double(0.0), C.c_int(0)
        self._chk(self._L.cvh_sync(self._h, C.byref(done), C.byref(nrm), C.byref(stopped)))
        return done.value, nrm.value, bool(stopped.value)

    def reset_run(self):
        self._chk(self._L.cvh_reset_run(self._h))

    def get_means(self):
        c1, c2 = np.zeros(3), np.zeros(3)
        self._chk(self._L.cvh_get_means(self._h, _dp(c1), _dp(c2)))
        return c1[:self.channels].copy(), c2[:self.channels].copy()

    def energy(self):
        """cvh_energy: the Chan-Sandberg-Vese functional of the current level set, term by term, evaluated on the device (Energy).
        Only reads: a run continued after it is bit-identical to one without."""
        t = EnergyTerms()
        _check(self._L.cvh_energy(self._h, C.byref(t)))
        return _energy_of(t, self.channels)

    def score(self, truth, invert=False, tol=2.0, stream=0):
        """cvh_score_mask / cvh_score_mask_device: the mask of the current level set against a ground truth (non-zero = foreground),
        scored on the device (Score): overlap counts, surface sizes and the exact surface distances.  truth is a numpy array of
        (h, w) -- bool or uint8, staged by the library -- or the integer address of h * w bytes in device memory, ordered behind
        `stream`; tol is the surface tolerance in pixels (tol2 = floor(tol^2)).  Only reads: a run continued after it is bit-identical
        to one without."""
        s, tol2 = MaskScore(), score_tol2(tol)
        if isinstance(truth, np.ndarray):
            t = np.ascontiguousarray(truth.view(np.uint8) if truth.dtype == np.bool_ else truth, dtype=np.uint8)
            assert t.shape == (self.h, self.w)
            _check(self._L.cvh_score_mask(self._h, _u8p(t), int(bool(invert)), tol2, C.byref(s)))
        else:
            _check(self._L.cvh_score_mask_device(self._h, _ptr(truth), int(bool(invert)), tol2, C.byref(s), _ptr(stream)))
        return _score_of(s)

    def get_trace(self, max_rows):
        out = np.zeros((max(max_rows, 1), 2 * self.channels + 1), dtype=np.float64)
        rows = C.c_int(0)
        self._chk(self._L.cvh_get_trace(self._h, _dp(out), int(max_rows), C.byref(rows)))
        return out[:rows.value].copy()

    def localized_means(self, radius, want=("c1", "c2", "wq", "a", "s")):
        """cvh_localized_means: the local means of the CURRENT level set and the integer sums they are quotients of, as a dict of the
        planes named in `want`: c1, c2 float64 (C, h, w); wq, a uint64 (h, w); s uint64 (C, h, w).  Only reads."""
        shapes = {"c1": (np.float64, True), "c2": (np.float64, True), "wq": (np.uint64, False), "a": (np.uint64, False), "s": (np.uint64, True)}
        out = {k: np.zeros((self.channels, self.h, self.w) if shapes[k][1] else (self.h, self.w), dtype=shapes[k][0]) for k in want}
        ptr = lambda k, cast: cast(out[k]) if k in out else None
        addr = lambda a: a.ctypes.data
        self._chk(self._L.cvh_localized_means(self._h, int(radius), ptr("c1", _dp), ptr("c2", _dp), ptr("wq", addr), ptr("a", addr), ptr("s", addr)))
        return out

    def set_edge_map(self, gq, stream=0):
        """cvh_set_edge_map / cvh_set_edge_map_device: the context's edge plane, g = gq 2^-15, from a numpy array of (h, w) uint16
        values 0 .. 32768 (above: refused), or from the integer address of h * w uint16 in device memory, ordered behind `stream`
        (above 32768: clamped on the device)."""
        if isinstance(gq, np.ndarray):
            if gq.dtype != np.uint16 or gq.shape != (self.h, self.w):   # (no conversion: a wider integer would wrap, a float truncate)
                raise ValueError(f"set_edge_map: a uint16 array of shape {(self.h, self.w)}, got {gq.dtype} {gq.shape}")
            a = np.ascontiguousarray(gq)
            self._chk(self._L.cvh_set_edge_map(self._h, a.ctypes.data))
        elif isinstance(gq, (int, np.integer)) and not isinstance(gq, bool):
            self._chk(self._L.cvh_set_edge_map_device(self._h, _ptr(gq), _ptr(stream)))
        else:
            raise ValueError(f"set_edge_map: a uint16 numpy array or the integer address of device memory, got {type(gq).__name__}")

    def get_edge_map(self, ptr=0, stream=0):
        """cvh_get_edge_map / cvh_get_edge_map_device: the edge plane as a uint16 array of (h, w), or written to device memory at `ptr`."""
        if ptr:
            self._chk(self._L.cvh_get_edge_map_device(self._h, int(ptr), _ptr(stream)))
            return None
        out = np.empty((self.h, self.w), dtype=np.uint16)
        self._chk(self._L.cvh_get_edge_map(self._h, out.ctypes.data))
        return out

    def relaxed(self, duals=False, ptr=0, stream=0):
        """cvh_get_relaxed / cvh_get_relaxed_device: v of the context's relaxation state as a float64 array of (h, w) -- with duals
        (v, qx, qy) --, or v written to device memory at `ptr`, ordered behind `stream`."""
        if ptr:
            self._chk(self._L.cvh_get_relaxed_device(self._h, int(ptr), _ptr(stream)))
            return None
        out = [np.empty((self.h, self.w), dtype=np.float64) for _ in range(3 if duals else 1)]
        self._chk(self._L.cvh_get_relaxed(self._h, *[_dp(a) for a in out], *([None] * (3 - len(out)))))
        return tuple(out) if duals else out[0]

    def edge_map_from(self, src, K):
        """cvh_edge_map: this context's edge plane from the planes of `src` (may be self) as they are now:
        gq = rint(32768 / (1 + |Sobel gradient|^2 / (64 C K^2))).  Smooth first (perona_malik, or a local mean in a second context)."""
        _check(self._L.cvh_edge_map(self._h, src._h, float(K)))

    def multiphase_labels_with(self, b, ptr=0, stream=0):
        """cvh_multiphase_labels / _device: label = mask(self) + 2 mask(b) per pixel, one launch.  Returns a uint8 array of (h, w), or
        with ptr (an integer device address of h * w bytes, ordered behind `stream`) writes there without a host wait.  Only reads."""
        if ptr:
            _check(self._L.cvh_multiphase_labels_device(self._h, b._h, int(ptr), _ptr(stream)))
            return None
        out = np.empty((self.h, self.w), dtype=np.uint8)
        _check(self._L.cvh_multiphase_labels(self._h, b._h, _u8p(out)))
        return out

    def get_stop_condition(self):
        v = C.c_double(0.0)
        self._chk(self._L.cvh_get_stop_condition(self._h, C.byref(v)))
        return v.value

    def get_mask(self, invert=False):
        m = np.empty((self.h, self.w), dtype=np.uint8)
        self._chk(self._L.cvh_get_mask(self._h, _u8p(m), int(bool(invert))))
        return m

    def components(self, conn=4, invert=False, labels_ptr=0, stream=0, cap=None):
        """cvh_components: label the connected components of the mask on the device.  labels_ptr: integer device address of h * w int32
        (0 = no label plane).  Returns (K, table): table is a structured array (COMPONENT_DTYPE) of the first min(K, cap) rows;
        cap = None asks for all K rows and COSTS TWO LABELLINGS (one call for K and the labels, a second one with cap = K for the rows: the
        host table must exist before the call that fills it); pass a cap where an upper bound of K is known, cap = 0 for no table."""
        count = C.c_int(0)

        def call(table, cap_):
            rows_only = cap is None and table is not None   # (the second of two calls: no label plane again, and no stream)
            self._chk(self._L.cvh_components(self._h, int(conn), int(bool(invert)), None if rows_only else _ptr(labels_ptr), table, cap_,
                                             C.byref(count), None if rows_only else _ptr(stream)))
            return count.value
        return _count_then_rows(call, COMPONENT_DTYPE, cap)

    def measure(self, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, cap=None, stream=0):
        """cvh_measure: the components of the mask -- get_mask_clean's for the same five options, (0, 0, False) the raw one -- measured
        on the device.  Returns (K, table): table is a structured array (REGION_DTYPE) of the first min(K, cap) rows: first, area, box,
        border, perimeter, coordinate sums and the sums of the image planes and their squares (region_shapes derives centroid, moments,
        axes, mean and variance).  cap = None asks for all K rows and COSTS TWO LABELLINGS (as components); pass a cap where an upper
        bound of K is known, cap = 0 for the count alone.  Only reads: a run continued after it is bit-identical to one without."""
        count = C.c_int(0)
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest)

        def call(table, cap_):
            _check(self._L.cvh_measure(self._h, *args, table, cap_, C.byref(count), _ptr(stream)))
            return count.value
        return _count_then_rows(call, REGION_DTYPE, cap)

    def overlaps(self, other, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, cap=None, stream=0):
        """cvh_overlaps / cvh_overlaps_device: the contingency table of the mask's components -- measure's for the same five options --
        against a second label plane, on the device.  other is a numpy array of (h, w), taken as int32 and staged by the library, or
        the integer address of h * w int32 in device memory (for instance the label plane components() wrote for the previous frame),
        ordered behind `stream`.  Returns (rows, K): rows a structured array (OVERLAP_DTYPE) of the first min(P, cap) rows (a, b, count),
        sorted by a, then by b as signed integers, the rows with a = 0 or b = 0 included; cap = None asks for all P rows and COSTS TWO
        CALLS (as measure); cap = 0 gives K alone.  Only reads: a run continued after it is bit-identical to one without."""
        pairs, count = C.c_long(0), C.c_int(0)
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest)
        if isinstance(other, np.ndarray):
            plane = np.ascontiguousarray(other, dtype=np.int32)
            assert plane.shape == (self.h, self.w)

            def call(table, cap_):
                _check(self._L.cvh_overlaps(self._h, *args, plane.ctypes.data, table, cap_, C.byref(pairs), C.byref(count)))
                return pairs.value
        else:
            def call(table, cap_):
                _check(self._L.cvh_overlaps_device(self._h, *args, _ptr(other), table, cap_, C.byref(pairs), C.byref(count),
                                                       _ptr(stream)))
                return pairs.value
        _, rows = _rows(call, OVERLAP_DTYPE, call(None, 0) if cap is None else cap)   # (the rows are asked for even where the count is 0)
        return rows, count.value

    def contour_counts(self, conn=8, invert=False, min_area=0, fill_holes=0, keep_largest=False, simplify=True):
        """cvh_contours without outputs: (nloops, npoints) of the boundary of the mask."""
        nloops, npoints = C.c_long(0), C.c_long(0)
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (int(bool(simplify)),)
        _check(self._L.cvh_contours(self._h, *args, None, 0, None, 0, C.byref(nloops), C.byref(npoints)))
        return nloops.value, npoints.value

    def contours(self, conn=8, invert=False, min_area=0, fill_holes=0, keep_largest=False, simplify=True):
        """cvh_contours: the boundary of the mask -- get_mask_clean's for the same five options, (0, 0, False) the raw one -- as ordered
        closed loops of lattice points, traced on the device.  Returns (loops, points): loops a structured array (CONTOUR_LOOP_DTYPE:
        first, edges, points, offset, area2 -- twice the enclosed area, negative for a hole), points an int32 array (P, 2) of x, y;
        loop k's points are points[offset : offset + points] in cycle order, the foreground on their right.  simplify keeps the corners
        only.  COSTS TWO TRACES (the counts size the arrays).  Only reads: a run continued after it is bit-identical to one without."""
        nl, npts = self.contour_counts(conn, invert, min_area, fill_holes, keep_largest, simplify)
        loops, points = np.zeros(nl, dtype=CONTOUR_LOOP_DTYPE), np.zeros((npts, 2), dtype=np.int32)
        if nl:
            nloops, npoints = C.c_long(0), C.c_long(0)
            args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (int(bool(simplify)),)
            _check(self._L.cvh_contours(self._h, *args, loops.ctypes.data, nl, points.ctypes.data, npts, C.byref(nloops), C.byref(npoints)))
        return loops, points

    def contours_subpixel(self, conn=8, invert=False, min_area=0, fill_holes=0, keep_largest=False):
        """cvh_contours_subpixel: the zero level of the level set as ordered closed polygons -- the loops of contours(simplify=False) for
        the same five options, each lattice point replaced by the point where u changes sign across that edge (the edge's midpoint
        where it does not: the plane's border, a pixel cleaning reclassified, NaN, zeros, infinities).  Returns (loops, points): loops
        as contours() gives them with simplify=False, points a float64 array (P, 2) of x, y with pixel centres at half-integers.
        COSTS TWO TRACES (the counts size the arrays).  Only reads: a run continued after it is bit-identical to one without."""
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest)
        nloops, npoints = C.c_long(0), C.c_long(0)
        _check(self._L.cvh_contours_subpixel(self._h, *args, None, 0, None, 0, C.byref(nloops), C.byref(npoints)))
        nl, npts = nloops.value, npoints.value
        loops, points = np.zeros(nl, dtype=CONTOUR_LOOP_DTYPE), np.zeros((npts, 2), dtype=np.float64)
        if nl:
            _check(self._L.cvh_contours_subpixel(self._h, *args, loops.ctypes.data, nl, points.ctypes.data, npts, C.byref(nloops), C.byref(npoints)))
        return loops, points

    def get_mask_clean(self, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False):
        """cvh_get_mask_clean: the mask without foreground components below min_area, with the holes of area <= fill_holes filled
        (-1: any size) and, with keep_largest, only its largest component; (0, 0, False) is get_mask."""
        m = np.empty((self.h, self.w), dtype=np.uint8)
        self._chk(self._L.cvh_get_mask_clean(self._h, _u8p(m), int(conn), int(bool(invert)), int(min_area), int(fill_holes), int(keep_largest)))
        return m

    def get_mask_clean_device(self, ptr, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, stream=0):
        self._chk(self._L.cvh_get_mask_clean_device(self._h, _ptr(ptr), int(conn), int(bool(invert)), int(min_area), int(fill_holes),
                                                    int(keep_largest), _ptr(stream)))

    def mask_morph(self, op, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, out=None, stream=0):
        """cvh_get_mask_morph / cvh_get_mask_morph_device: the cleaned mask (get_mask_clean's arguments) dilated, eroded, opened or closed
        by the disk dx^2 + dy^2 <= r2 (or radius: r2 = floor(radius^2)) on the device; op is a MORPH_* code or its name.  out is None (a
        new (h, w) uint8 array is returned), a contiguous uint8 array of (h, w) to fill, or the integer address of h * w bytes in device
        memory, written behind what `stream` holds.  Only reads: a run continued after it is bit-identical to one without."""
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (morph_code(op), _morph_r2(r2, radius))
        if out is None or isinstance(out, np.ndarray):
            m = np.empty((self.h, self.w), dtype=np.uint8) if out is None else out
            assert m.dtype == np.uint8 and m.shape == (self.h, self.w) and m.flags["C_CONTIGUOUS"]
            _check(self._L.cvh_get_mask_morph(self._h, _u8p(m), *args))
            return m
        _check(self._L.cvh_get_mask_morph_device(self._h, _ptr(out), *args, _ptr(stream)))
        return out

    def split(self, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, labels_ptr=0, cap=None, stream=0):
        """cvh_split: the cleaned mask (get_mask_clean's arguments) taken apart into one object per core of its erosion by the disk
        dx^2 + dy^2 <= r2 (r2, or radius with r2 = floor(radius^2)): "Object split" in include/chanvese_hip.h.  labels_ptr: integer device
        address of h * w int32 (0 = no label plane).  Returns (labels, table, K): labels is labels_ptr or None; table is a structured array
        (COMPONENT_DTYPE) of the first min(K, cap) rows -- `first` the marker's smallest flat index, area and box those of the grown
        object.  cap = None asks for all K rows and COSTS TWO CALLS (as components); cap = 0 for no table.  Only reads."""
        count = C.c_int(0)
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (_morph_r2(r2, radius),)
        labels = _ptr(labels_ptr)

        def call(table, cap_):
            rows_only = cap is None and table is not None   # (as in components)
            _check(self._L.cvh_split(self._h, *args, None if rows_only else labels, table, cap_, C.byref(count), None if rows_only else _ptr(stream)))
            return count.value
        k, table = _count_then_rows(call, COMPONENT_DTYPE, cap)
        return labels, table, k

    def split_labels(self, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False):
        """cvh_split_host: split()'s label plane as a numpy int32 array (h, w) in host memory, and K: (labels, K)."""
        count = C.c_int(0)
        labels = np.empty((self.h, self.w), dtype=np.int32)
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (_morph_r2(r2, radius),)
        _check(self._L.cvh_split_host(self._h, *args, labels.ctypes.data, None, 0, C.byref(count)))
        return labels, count.value

    def split_levelset(self, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, inside=1.0, outside=-1.0):
        """cvh_split_levelset: split in place -- the level set becomes `inside` on the split objects and `outside` on the cut lines and the
        background, and a new run begins; components, measure, contours, overlaps and further iterations then see the split objects."""
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (_morph_r2(r2, radius),)
        _check(self._L.cvh_split_levelset(self._h, *args, float(inside), float(outside)))

    def morph_levelset(self, op, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, inside=1.0,
                       outside=-1.0):
        """cvh_morph_levelset: mask_morph in place -- the level set becomes `inside` where that mask is 1 and `outside` elsewhere, and a
        new run begins as after set_levelset; the mask never leaves the device.  With MORPH_NONE the cleaned mask is baked in."""
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (morph_code(op), _morph_r2(r2, radius))
        _check(self._L.cvh_morph_levelset(self._h, *args, float(inside), float(outside)))

    def init_mask(self, mask, inside=1.0, outside=-1.0, stream=0):
        """cvh_init_mask / cvh_init_mask_device: u = inside where the mask's byte is nonzero, outside elsewhere, written on the device (one
        byte per pixel crosses, not eight); the context is left as set_levelset of those doubles leaves it.  mask is a numpy array of
        (h, w), bool or uint8, or the integer address of h * w bytes in device memory, read behind what `stream` holds.  Needs neither
        an image nor a level set."""
        if isinstance(mask, np.ndarray):
            m = np.ascontiguousarray(mask.view(np.uint8) if mask.dtype == np.bool_ else mask, dtype=np.uint8)
            assert m.shape == (self.h, self.w)
            _check(self._L.cvh_init_mask(self._h, _u8p(m), float(inside), float(outside)))
        else:
            _check(self._L.cvh_init_mask_device(self._h, _ptr(mask), float(inside), float(outside), _ptr(stream)))

    def get_contour(self):
        m = np.empty((self.h, self.w), dtype=np.uint8)
        self._chk(self._L.cvh_get_contour(self._h, _u8p(m)))
        return m

    def separate(self, img3, invert=False):
        img3 = np.ascontiguousarray(img3, dtype=np.uint8)
        assert img3.shape == (self.h, self.w, 3)
        out = np.empty_like(img3)
        self._chk(self._L.cvh_separate(self._h, _u8p(img3), int(bool(invert)), _u8p(out)))
        return out

    def perona_malik(self, K=10.0, L=0.25, T=20.0):
        self._chk(self._L.cvh_perona_malik(self._h, float(K), float(L), float(T)))

    def last_run_ms(self):
        v = C.c_float(0.0)
        self._chk(self._L.cvh_last_run_ms(self._h, C.byref(v)))
        return v.value

    def launch_info(self, phase=0):
        """What the library launches (phase 0: the CSV step with the current options; 1: the last Perona-Malik call) as a
        dict of the key=value pairs cvh_launch_info writes; "kernel" is the instantiation as rocprofv3 prints it."""
        buf = C.create_string_buffer(512)
        self._chk(self._L.cvh_launch_info(self._h, int(phase), buf, len(buf)))
        out = {}
        for tok in buf.value.decode().split(" "):
            if "=" in tok:
                k, v = tok.split("=", 1)
                out[k] = v
            elif out:                       # template arguments are separated by ", "
                last = next(reversed(out))
                out[last] += " " + tok
        return out

    def last_pm_ms(self):
        v = C.c_float(0.0)
        self._chk(self._L.cvh_last_pm_ms(self._h, C.byref(v)))
        return v.value
