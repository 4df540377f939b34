"""ctypes binding of include/chanvese_hip.h (the C ABI of libchanvese_hip.so).

No CPU fallback: if the HIP library has not been built, importing/using this module raises
with instructions.  In a process that also imports torch, import torch FIRST: torch ships
its own libamdhip64.so.7 and the loader then shares that one runtime with this library.
"""
import ctypes as C
import dataclasses
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CHANVESE_HIP_LIB selects another BUILD of the same library (A/B variants under csrc/variants/, tools/build_variant.sh)
LIB_PATH = os.environ.get("CHANVESE_HIP_LIB") or os.path.join(_HERE, "csrc", "libchanvese_hip.so")

CVH_OK = 0
OP_DELTA, OP_HEAVISIDE, OP_ONE_MINUS_HEAVISIDE = 0, 1, 2
MATH_DEFAULT, MATH_STRICT, MATH_FAST = 0, 1, 2

# every symbol include/chanvese_hip.h declares
EXPORTS = [
    "cvh_default_params", "cvh_device_count", "cvh_create", "cvh_destroy", "cvh_last_error",
    "cvh_set_params", "cvh_set_option", "cvh_set_image", "cvh_get_image", "cvh_set_levelset",
    "cvh_get_levelset", "cvh_init_checkerboard", "cvh_levelset_checkerboard_host", "cvh_run",
    "cvh_enqueue_steps", "cvh_warm", "cvh_sync", "cvh_reset_run", "cvh_get_means", "cvh_get_trace",
    "cvh_get_stop_condition", "cvh_get_mask", "cvh_get_contour", "cvh_separate", "cvh_perona_malik",
    "cvh_pm_trip_count", "cvh_last_run_ms", "cvh_last_pm_ms", "cvh_ppf_apply",
    "cvh_ppf_apply_device", "cvh_version", "cvh_launch_info", "cvh_enqueue_steps_batch", "cvh_run_batch",
    "cvh_perona_malik_batch",
    "cvh_set_image_device", "cvh_get_image_device", "cvh_set_levelset_device", "cvh_get_levelset_device",
    "cvh_get_mask_device", "cvh_set_image_device_batch", "cvh_init_checkerboard_batch", "cvh_get_mask_device_batch",
    "cvh_reinit", "cvh_reinit_batch",
    "cvh_components", "cvh_components_batch", "cvh_get_mask_clean", "cvh_get_mask_clean_device", "cvh_get_mask_clean_device_batch",
    "cvh_histogram", "cvh_histogram_batch", "cvh_otsu_from_histogram", "cvh_otsu_threshold", "cvh_init_threshold", "cvh_init_threshold_batch",
    "cvh_init_otsu", "cvh_init_otsu_batch", "cvh_init_rect", "cvh_init_rect_batch", "cvh_init_disk", "cvh_init_disk_batch",
    "cvh_restrict_image", "cvh_restrict_image_batch", "cvh_prolong_levelset", "cvh_prolong_levelset_batch",
    "cvh_convert_colour", "cvh_convert_colour_batch", "cvh_luma_image", "cvh_luma_image_batch",
    "cvh_local_planes", "cvh_local_planes_batch",
    "cvh_rank_planes", "cvh_rank_planes_batch",
    "cvh_energy", "cvh_energy_batch",
    "cvh_score_mask", "cvh_score_mask_device", "cvh_score_mask_device_batch",
    "cvh_measure", "cvh_measure_batch", "cvh_region_shape_of",
    "cvh_overlaps", "cvh_overlaps_device", "cvh_overlaps_device_batch", "cvh_match_overlaps",
    "cvh_contours", "cvh_contours_device", "cvh_contours_device_batch",
    "cvh_contours_subpixel", "cvh_contours_subpixel_device", "cvh_contours_subpixel_device_batch", "cvh_contour_subpixel_measure",
    "cvh_get_mask_morph", "cvh_get_mask_morph_device", "cvh_get_mask_morph_device_batch", "cvh_morph_levelset", "cvh_morph_levelset_batch",
    "cvh_init_mask", "cvh_init_mask_device", "cvh_init_mask_device_batch",
    "cvh_split", "cvh_split_host", "cvh_split_batch", "cvh_split_levelset", "cvh_split_levelset_batch", "cvh_split_geometry",
    "cvh_multiphase_run", "cvh_multiphase_run_batch", "cvh_multiphase_means", "cvh_multiphase_labels", "cvh_multiphase_labels_device", "cvh_multiphase_geometry",
    "cvh_localized_run", "cvh_localized_run_batch", "cvh_localized_means", "cvh_localized_geometry",
    "cvh_set_edge_map", "cvh_get_edge_map", "cvh_set_edge_map_device", "cvh_get_edge_map_device", "cvh_edge_map", "cvh_edge_map_batch",
    "cvh_geodesic_run", "cvh_geodesic_run_batch", "cvh_geodesic_geometry",
]
# "Mask morphology": the operations of cvh_get_mask_morph* / cvh_morph_levelset*, by code and by name
MORPH_NONE, MORPH_DILATE, MORPH_ERODE, MORPH_OPEN, MORPH_CLOSE = 0, 1, 2, 3, 4
MORPH_OPS = {"none": MORPH_NONE, "dilate": MORPH_DILATE, "erode": MORPH_ERODE, "open": MORPH_OPEN, "close": MORPH_CLOSE}
# struct cvh_component: row k - 1 of a component table describes label k (first = smallest flat index; the box is inclusive)
COMPONENT_DTYPE = np.dtype([("first", np.uint32), ("area", np.uint32), ("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32)])
# struct cvh_region (128 bytes): row k - 1 of a measure table describes label k ("Component measures" in include/chanvese_hip.h)
REGION_DTYPE = np.dtype([("first", np.uint32), ("area", np.uint32), ("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32),
                         ("border", np.uint32), ("reserved", np.uint32)] +
                        [(f, np.uint64) for f in ("perimeter", "sx", "sy", "sxx", "syy", "sxy")] + [("s1", np.uint64, 3), ("s2", np.uint64, 3)])
# struct cvh_region_shape: what cvh_region_shape_of derives from a row
REGION_SHAPE_DTYPE = np.dtype([(f, np.float64) for f in ("cx", "cy", "mu20", "mu02", "mu11", "theta", "major", "minor")] +
                              [("mean", np.float64, 3), ("var", np.float64, 3)])
# struct cvh_contour_loop (32 bytes): one closed loop of the mask's boundary ("Contours" in include/chanvese_hip.h)
CONTOUR_LOOP_DTYPE = np.dtype([("first", np.uint32), ("edges", np.uint32), ("points", np.uint32), ("pad", np.uint32), ("offset", np.uint64),
                               ("area2", np.int64)])
# struct cvh_overlap (16 bytes): one row of the contingency table ("Component overlaps" in include/chanvese_hip.h)
OVERLAP_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("count", np.uint32), ("pad", np.uint32)])
LAYOUT_PLANAR, LAYOUT_INTERLEAVED = 0, 1
# "Colour spaces": which plane is which primary, and the spaces cvh_convert_colour knows
ORDERS = {"bgr": 0, "rgb": 1}
COLOUR_SPACES = {"ycrcb": 1, "yuv": 2}
# "Local statistics": what plane k of the destination of cvh_local_planes becomes, by code and -- whole tuples -- by name
LOCAL_COPY, LOCAL_MEAN, LOCAL_DEV = 0, 1, 2
LOCAL_RADIUS_MAX = 127
LOCAL_WHATS = {"mean": (LOCAL_MEAN,) * 3, "dev": (LOCAL_DEV,) * 3, "stack": (LOCAL_COPY, LOCAL_MEAN, LOCAL_DEV)}
# "Rank planes": what plane k of the destination of cvh_rank_planes becomes, by code and -- every plane alike -- by name
RANK_COPY, RANK_MIN, RANK_MAX, RANK_MEDIAN, RANK_OPEN, RANK_CLOSE, RANK_TOPHAT, RANK_BOTHAT = range(8)
RANK_RADIUS_MAX, RANK_MEDIAN_RADIUS_MAX = 127, 7
RANK_WHATS = {"min": RANK_MIN, "max": RANK_MAX, "median": RANK_MEDIAN, "open": RANK_OPEN, "close": RANK_CLOSE, "tophat": RANK_TOPHAT,
              "bothat": RANK_BOTHAT}


class Params(C.Structure):
    """struct cvh_params (src/main.cpp:731-734 of the reference)."""
    _fields_ = [("mu", C.c_double), ("nu", C.c_double), ("dt", C.c_double),
                ("eps", C.c_double), ("tol", C.c_double),
                ("lambda1", C.c_double * 3), ("lambda2", C.c_double * 3)]


class EnergyTerms(C.Structure):
    """struct cvh_energy_terms ("Energy" in include/chanvese_hip.h)."""
    _fields_ = [("total", C.c_double), ("length", C.c_double), ("area", C.c_double),
                ("fit_in", C.c_double * 3), ("fit_out", C.c_double * 3), ("c1", C.c_double * 3), ("c2", C.c_double * 3)]


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


class MaskScore(C.Structure):
    """struct cvh_mask_score ("Mask scores" in include/chanvese_hip.h)."""
    _fields_ = [(f, C.c_uint64) for f in ("tp", "fp", "fn", "tn", "surf_m", "surf_t", "within_m", "within_t", "dist_m_q16", "dist_t_q16")] + \
               [("hd2_m", C.c_uint32), ("hd2_t", C.c_uint32), ("defined", C.c_int32), ("pad", C.c_int32)]


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


class Match(C.Structure):
    """struct cvh_match ("Component overlaps" in include/chanvese_hip.h)."""
    _fields_ = [(f, C.c_uint32) for f in ("objects_a", "objects_b", "tp", "fp", "fn", "pad")]


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


class CvhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"chanvese_hip error {code}: {msg}")
        self.code = code


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C chan_vese_amd/csrc). "
            "There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    dp, u8p, ip = C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int)
    u8pp, vp, lp = C.POINTER(u8p), C.c_void_p, C.POINTER(C.c_long)
    sig = {
        "cvh_default_params": (None, [C.POINTER(Params)]),
        "cvh_device_count": (C.c_int, [ip]),
        "cvh_create": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(Params), C.c_int]),
        "cvh_destroy": (None, [vp]),
        "cvh_last_error": (C.c_char_p, [vp]),
        "cvh_set_params": (C.c_int, [vp, C.POINTER(Params)]),
        "cvh_set_option": (C.c_int, [vp, C.c_char_p, C.c_long]),
        "cvh_set_image": (C.c_int, [vp, u8pp]),
        "cvh_get_image": (C.c_int, [vp, u8pp]),
        "cvh_set_levelset": (C.c_int, [vp, dp]),
        "cvh_get_levelset": (C.c_int, [vp, dp]),
        "cvh_init_checkerboard": (C.c_int, [vp]),
        "cvh_levelset_checkerboard_host": (None, [C.c_int, C.c_int, dp]),
        "cvh_run": (C.c_int, [vp, C.c_int, ip, dp]),
        "cvh_enqueue_steps": (C.c_int, [vp, C.c_int]),
        "cvh_warm": (C.c_int, [vp, C.c_int]),
        "cvh_sync": (C.c_int, [vp, ip, dp, ip]),
        "cvh_reset_run": (C.c_int, [vp]),
        "cvh_get_means": (C.c_int, [vp, dp, dp]),
        "cvh_get_trace": (C.c_int, [vp, dp, C.c_int, ip]),
        "cvh_get_stop_condition": (C.c_int, [vp, dp]),
        "cvh_get_mask": (C.c_int, [vp, u8p, C.c_int]),
        "cvh_get_contour": (C.c_int, [vp, u8p]),
        "cvh_separate": (C.c_int, [vp, u8p, C.c_int, u8p]),
        "cvh_perona_malik": (C.c_int, [vp, C.c_double, C.c_double, C.c_double]),
        "cvh_pm_trip_count": (C.c_int, [C.c_double, C.c_double]),
        "cvh_last_run_ms": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "cvh_last_pm_ms": (C.c_int, [vp, C.POINTER(C.c_float)]),
        "cvh_ppf_apply": (C.c_int, [dp, C.c_int, C.c_long, C.c_long, C.c_int, C.c_double, C.c_int]),
        "cvh_ppf_apply_device": (C.c_int, [dp, C.c_long, C.c_int, C.c_double, vp]),
        "cvh_version": (C.c_char_p, []),
        "cvh_launch_info": (C.c_int, [vp, C.c_int, C.c_char_p, C.c_int]),
        "cvh_enqueue_steps_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int]),
        "cvh_run_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, ip, dp]),
        "cvh_perona_malik_batch": (C.c_int, [C.POINTER(vp), C.c_int, dp, dp, dp]),
        "cvh_set_image_device": (C.c_int, [vp, vp, C.c_int, vp]),
        "cvh_get_image_device": (C.c_int, [vp, vp, C.c_int, vp]),
        "cvh_set_levelset_device": (C.c_int, [vp, vp, C.c_int, vp]),
        "cvh_get_levelset_device": (C.c_int, [vp, vp, C.c_int, vp]),
        "cvh_get_mask_device": (C.c_int, [vp, vp, C.c_int, vp]),
        "cvh_set_image_device_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, vp]),
        "cvh_init_checkerboard_batch": (C.c_int, [C.POINTER(vp), C.c_int]),
        "cvh_get_mask_device_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, vp]),
        "cvh_reinit": (C.c_int, [vp, ip]),
        "cvh_reinit_batch": (C.c_int, [C.POINTER(vp), C.c_int, ip]),
        "cvh_components": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, C.c_int, ip, vp]),
        "cvh_components_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(vp), ip, vp]),
        "cvh_get_mask_clean": (C.c_int, [vp, u8p, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int]),
        "cvh_get_mask_clean_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, vp]),
        "cvh_get_mask_clean_device_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, vp]),
        "cvh_histogram": (C.c_int, [vp, vp, C.c_int, ip]),
        "cvh_histogram_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(vp), ip]),
        "cvh_otsu_from_histogram": (C.c_int, [vp, C.c_int, ip]),
        "cvh_otsu_threshold": (C.c_int, [vp, ip]),
        "cvh_init_threshold": (C.c_int, [vp, C.c_int, C.c_double, C.c_double]),
        "cvh_init_threshold_batch": (C.c_int, [C.POINTER(vp), C.c_int, ip, C.c_double, C.c_double]),
        "cvh_init_otsu": (C.c_int, [vp, ip, C.c_double, C.c_double]),
        "cvh_init_otsu_batch": (C.c_int, [C.POINTER(vp), C.c_int, ip, C.c_double, C.c_double]),
        "cvh_init_rect": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]),
        "cvh_init_rect_batch": (C.c_int, [C.POINTER(vp), C.c_int, ip, C.c_double, C.c_double]),
        "cvh_init_disk": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]),
        "cvh_init_disk_batch": (C.c_int, [C.POINTER(vp), C.c_int, ip, C.c_double, C.c_double]),
        "cvh_restrict_image": (C.c_int, [vp, vp]),
        "cvh_restrict_image_batch": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.c_int]),
        "cvh_prolong_levelset": (C.c_int, [vp, vp]),
        "cvh_prolong_levelset_batch": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.c_int]),
        "cvh_convert_colour": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
        "cvh_convert_colour_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int]),
        "cvh_luma_image": (C.c_int, [vp, vp, C.c_int]),
        "cvh_luma_image_batch": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int]),
        "cvh_local_planes": (C.c_int, [vp, vp, C.c_int, ip]),
        "cvh_local_planes_batch": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.c_int, ip, ip]),
        "cvh_rank_planes": (C.c_int, [vp, vp, C.c_int, ip]),
        "cvh_rank_planes_batch": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.c_int, ip, ip]),
        "cvh_energy": (C.c_int, [vp, C.POINTER(EnergyTerms)]),
        "cvh_energy_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(EnergyTerms)]),
        "cvh_score_mask": (C.c_int, [vp, u8p, C.c_int, C.c_uint32, C.POINTER(MaskScore)]),
        "cvh_score_mask_device": (C.c_int, [vp, vp, C.c_int, C.c_uint32, C.POINTER(MaskScore), vp]),
        "cvh_score_mask_device_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, C.c_uint32, C.POINTER(MaskScore), vp]),
        "cvh_measure": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, vp, C.c_int, ip, vp]),
        "cvh_measure_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.POINTER(vp), ip, ip, vp]),
        "cvh_region_shape_of": (C.c_int, [vp, C.c_int, vp]),
        "cvh_overlaps": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, vp, vp, C.c_long, lp, ip]),
        "cvh_overlaps_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, vp, vp, C.c_long, lp, ip, vp]),
        "cvh_overlaps_device_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.POINTER(vp), C.POINTER(vp),
                                                lp, lp, ip, vp]),
        "cvh_match_overlaps": (C.c_int, [vp, C.c_long, C.c_uint32, C.c_uint32, vp, C.c_int, C.POINTER(Match)]),
        "cvh_contours": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, vp, C.c_long, vp, C.c_long, lp, lp]),
        "cvh_contours_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, vp, C.c_long, vp, C.c_long, lp, lp, vp]),
        "cvh_contours_device_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.POINTER(vp), lp,
                                                C.POINTER(vp), lp, lp, lp, vp]),
        "cvh_contours_subpixel": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, vp, C.c_long, vp, C.c_long, lp, lp]),
        "cvh_contours_subpixel_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, vp, C.c_long, vp, C.c_long, lp, lp, vp]),
        "cvh_contours_subpixel_device_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.POINTER(vp), lp,
                                                         C.POINTER(vp), lp, lp, lp, vp]),
        "cvh_contour_subpixel_measure": (C.c_int, [vp, C.c_long, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "cvh_get_mask_morph": (C.c_int, [vp, u8p, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_uint32]),
        "cvh_get_mask_morph_device": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_uint32, vp]),
        "cvh_get_mask_morph_device_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, C.c_int, C.c_long, C.c_long, C.c_int,
                                                      C.c_int, C.POINTER(C.c_uint32), vp]),
        "cvh_morph_levelset": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_uint32, C.c_double, C.c_double]),
        "cvh_morph_levelset_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_int,
                                               C.POINTER(C.c_uint32), C.c_double, C.c_double]),
        "cvh_init_mask": (C.c_int, [vp, u8p, C.c_double, C.c_double]),
        "cvh_init_mask_device": (C.c_int, [vp, vp, C.c_double, C.c_double, vp]),
        "cvh_init_mask_device_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_double, C.c_double, vp]),
        "cvh_split": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_uint32, vp, vp, C.c_int, ip, vp]),
        "cvh_split_host": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_uint32, vp, vp, C.c_int, ip]),
        "cvh_split_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.POINTER(C.c_uint32), C.POINTER(vp),
                                      ip, vp]),
        "cvh_split_levelset": (C.c_int, [vp, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.c_uint32, C.c_double, C.c_double]),
        "cvh_split_levelset_batch": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int, C.POINTER(C.c_uint32),
                                               C.c_double, C.c_double]),
        "cvh_split_geometry": (None, [ip, ip, ip]),
        "cvh_multiphase_run": (C.c_int, [vp, vp, C.c_int, ip, dp, dp, C.c_int, ip]),
        "cvh_multiphase_run_batch": (C.c_int, [vp, vp, C.c_int, C.c_int, ip, dp, vp, C.c_int, ip]),
        "cvh_multiphase_means": (C.c_int, [vp, vp, dp]),
        "cvh_multiphase_labels": (C.c_int, [vp, vp, u8p]),
        "cvh_multiphase_labels_device": (C.c_int, [vp, vp, vp, vp]),
        "cvh_multiphase_geometry": (None, [C.c_int, C.c_int, ip, ip, ip]),
        "cvh_localized_run": (C.c_int, [vp, C.c_int, C.c_int, ip, dp, dp, C.c_int, ip]),
        "cvh_localized_run_batch": (C.c_int, [vp, C.c_int, ip, C.c_int, ip, dp, vp, C.c_int, ip]),
        "cvh_localized_means": (C.c_int, [vp, C.c_int, dp, dp, vp, vp, vp]),
        "cvh_localized_geometry": (None, [C.c_int, C.c_int, C.c_int, ip, ip, ip, ip]),
        "cvh_set_edge_map": (C.c_int, [vp, vp]),
        "cvh_get_edge_map": (C.c_int, [vp, vp]),
        "cvh_set_edge_map_device": (C.c_int, [vp, vp, vp]),
        "cvh_get_edge_map_device": (C.c_int, [vp, vp, vp]),
        "cvh_edge_map": (C.c_int, [vp, vp, C.c_double]),
        "cvh_edge_map_batch": (C.c_int, [vp, vp, C.c_int, dp]),
        "cvh_geodesic_run": (C.c_int, [vp, C.c_int, ip, dp, dp, C.c_int, ip]),
        "cvh_geodesic_run_batch": (C.c_int, [vp, C.c_int, C.c_int, ip, dp, vp, C.c_int, ip]),
        "cvh_geodesic_geometry": (None, [C.c_int, C.c_int, ip, ip, ip]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


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
    rc = lib().cvh_ppf_apply(_dp(data), data.shape[1], start, end, int(op), float(eps), device)
    if rc != CVH_OK:
        raise CvhError(rc, lib().cvh_last_error(None).decode())
    return data


def _member_array(contexts):
    hs = [c._h.value for c in contexts]
    return (C.c_void_p * max(len(hs), 1))(*hs)


def enqueue_steps_batch(contexts, n):
    """Fused batch (cvh_enqueue_steps_batch): enqueues n iterations of every context with one launch per iteration and
    CSV-step instantiation; follow with sync() on each context, as after Context.enqueue_steps."""
    contexts = list(contexts)
    rc = lib().cvh_enqueue_steps_batch(_member_array(contexts), len(contexts), int(n))
    if rc != CVH_OK:
        raise CvhError(rc, lib().cvh_last_error(None).decode())


def run_batch(contexts, max_steps=-1):
    """Fused batch (cvh_run_batch): Context.run for every context at once, each with its own stop rule.
    Returns [(steps_done, last_norm)] per context."""
    contexts = list(contexts)
    n = len(contexts)
    done, nrm = (C.c_int * max(n, 1))(), (C.c_double * max(n, 1))()
    rc = lib().cvh_run_batch(_member_array(contexts), n, int(max_steps), done, nrm)
    if rc != CVH_OK:
        raise CvhError(rc, lib().cvh_last_error(None).decode())
    return [(done[i], nrm[i]) for i in range(n)]


def perona_malik_batch(contexts, K=10.0, L=0.25, T=20.0):
    """Perona-Malik batch (cvh_perona_malik_batch): Context.perona_malik for every context at once, the planes of several
    contexts sharing resident launches.  K, L and T are scalars (the same for every member) or sequences of one value per member."""
    contexts = list(contexts)
    n = len(contexts)

    def per_member(v, name):
        vals = [float(x) for x in v] if np.ndim(v) else [float(v)] * n
        if len(vals) != n:
            raise ValueError(f"{name}: {len(vals)} values for {n} members")
        return (C.c_double * max(n, 1))(*vals)

    k, l, t = per_member(K, "K"), per_member(L, "L"), per_member(T, "T")
    rc = lib().cvh_perona_malik_batch(_member_array(contexts), n, k, l, t)
    if rc != CVH_OK:
        raise CvhError(rc, lib().cvh_last_error(None).decode())


def _address_array(ptrs, n):
    if len(ptrs) != n:
        raise ValueError(f"{len(ptrs)} device pointers for {n} members")
    return (C.c_void_p * max(n, 1))(*[int(p) or None for p in ptrs])


def _batch_chk(rc):
    if rc != CVH_OK:
        raise CvhError(rc, lib().cvh_last_error(None).decode())


def set_image_device_batch(contexts, ptrs, layout=LAYOUT_PLANAR, stream=0):
    """cvh_set_image_device_batch: every context takes its image from device memory (ptrs: one integer address per context, uint8,
    planar or interleaved), one launch for all; ordered behind what `stream` (a HIP stream handle as integer, 0 = default) holds."""
    contexts = list(contexts)
    n = len(contexts)
    _batch_chk(lib().cvh_set_image_device_batch(_member_array(contexts), n, _address_array(list(ptrs), n), int(layout), int(stream) or None))


def init_checkerboard_batch(contexts):
    """cvh_init_checkerboard_batch: Context.init_checkerboard for every context with one copy and one launch."""
    contexts = list(contexts)
    _batch_chk(lib().cvh_init_checkerboard_batch(_member_array(contexts), len(contexts)))


def get_mask_device_batch(contexts, ptrs, invert=False, stream=0):
    """cvh_get_mask_device_batch: every context's mask into device memory (ptrs: one integer address of h * w bytes per context),
    one launch for all; work enqueued on `stream` afterwards sees the masks.  Does not block the host."""
    contexts = list(contexts)
    n = len(contexts)
    _batch_chk(lib().cvh_get_mask_device_batch(_member_array(contexts), n, _address_array(list(ptrs), n), int(bool(invert)), int(stream) or None))


def reinit_batch(contexts):
    """cvh_reinit_batch: Context.reinit for every context (any mix of shapes) with one set of launches.  Returns [changed] per context."""
    contexts = list(contexts)
    n = len(contexts)
    changed = (C.c_int * max(n, 1))()
    _batch_chk(lib().cvh_reinit_batch(_member_array(contexts), n, changed))
    return [bool(changed[i]) for i in range(n)]


def components_batch(contexts, ptrs=None, conn=4, invert=False, stream=0):
    """cvh_components_batch: the connected components of every context's mask with one set of launches.  ptrs: one integer device
    address of h * w int32 labels per context (0 = no label plane for that member), or None.  Returns [K] per context."""
    contexts = list(contexts)
    n = len(contexts)
    counts = (C.c_int * max(n, 1))()
    addr = None if ptrs is None else _address_array(list(ptrs), n)
    _batch_chk(lib().cvh_components_batch(_member_array(contexts), n, int(conn), int(bool(invert)), addr, counts, int(stream) or None))
    return [counts[i] for i in range(n)]


def get_mask_clean_device_batch(contexts, ptrs, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, stream=0):
    """cvh_get_mask_clean_device_batch: every context's cleaned mask (Context.get_mask_clean) into device memory, one set of launches
    for all; work enqueued on `stream` afterwards sees the masks.  Does not block the host."""
    contexts = list(contexts)
    n = len(contexts)
    _batch_chk(lib().cvh_get_mask_clean_device_batch(_member_array(contexts), n, _address_array(list(ptrs), n), int(conn), int(bool(invert)),
                                                     int(min_area), int(fill_holes), int(keep_largest), int(stream) or None))


def otsu_from_histogram(hist):
    """cvh_otsu_from_histogram: Otsu's threshold of a histogram of 1 .. 766 uint32 counts (the header's integer definition), on the host."""
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    t = C.c_int(-1)
    _batch_chk(lib().cvh_otsu_from_histogram(hist.ctypes.data, int(hist.size), C.byref(t)))
    return t.value


def _int_rows(values, n, width, name):
    """values: one row of `width` ints for all members, or a sequence of n rows -> a flat ctypes int array of n * width"""
    rows = [values] * n if (np.ndim(values) == (1 if width > 1 else 0)) else list(values)
    if len(rows) != n:
        raise ValueError(f"{name}: {len(rows)} values for {n} members")
    flat = []
    for r in rows:
        r = [r] if width == 1 else list(r)
        if len(r) != width:
            raise ValueError(f"{name}: {len(r)} numbers where {width} are needed")
        flat += [int(v) for v in r]
    return (C.c_int * max(len(flat), 1))(*flat)


def histogram_batch(contexts, caps=None):
    """cvh_histogram_batch: the grey histograms (g = the sum of the planes) of every context with one launch.  caps: bins wanted per
    member (None: all 255 C + 1).  Returns [uint32 array] per context."""
    contexts = list(contexts)
    n = len(contexts)
    caps = [255 * c.channels + 1 for c in contexts] if caps is None else [int(v) for v in caps]
    if len(caps) != n:
        raise ValueError(f"{len(caps)} capacities for {n} members")
    outs = [np.zeros(max(k, 0), dtype=np.uint32) for k in caps]
    ptrs = (C.c_void_p * max(n, 1))(*[o.ctypes.data if o.size else None for o in outs])
    _batch_chk(lib().cvh_histogram_batch(_member_array(contexts), n, ptrs, (C.c_int * max(n, 1))(*caps)))
    return [o[:min(o.size, 255 * c.channels + 1)] for o, c in zip(outs, contexts)]


def init_threshold_batch(contexts, t, inside=1.0, outside=-1.0):
    """cvh_init_threshold_batch: Context.init_threshold for every context with one launch; t is one int or one per member."""
    contexts = list(contexts)
    n = len(contexts)
    _batch_chk(lib().cvh_init_threshold_batch(_member_array(contexts), n, _int_rows(t, n, 1, "t"), float(inside), float(outside)))


def init_otsu_batch(contexts, inside=1.0, outside=-1.0):
    """cvh_init_otsu_batch: Context.init_otsu for every context: one histogram launch, one start launch.  Returns [t] per context."""
    contexts = list(contexts)
    n = len(contexts)
    t = (C.c_int * max(n, 1))()
    _batch_chk(lib().cvh_init_otsu_batch(_member_array(contexts), n, t, float(inside), float(outside)))
    return [t[i] for i in range(n)]


def init_rect_batch(contexts, xywh, inside=1.0, outside=0.0):
    """cvh_init_rect_batch: Context.init_rect for every context with one launch; xywh is (x, y, w, h) or one such row per member."""
    contexts = list(contexts)
    n = len(contexts)
    _batch_chk(lib().cvh_init_rect_batch(_member_array(contexts), n, _int_rows(xywh, n, 4, "xywh"), float(inside), float(outside)))


def init_disk_batch(contexts, cxcyr, inside=1.0, outside=0.0):
    """cvh_init_disk_batch: Context.init_disk for every context with one launch; cxcyr is (cx, cy, r) or one such row per member."""
    contexts = list(contexts)
    n = len(contexts)
    _batch_chk(lib().cvh_init_disk_batch(_member_array(contexts), n, _int_rows(cxcyr, n, 3, "cxcyr"), float(inside), float(outside)))


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
    _batch_chk(lib().cvh_restrict_image_batch(_member_array(fines), _member_array(coarses), len(fines)))


def prolong_levelset_batch(coarses, fines):
    """cvh_prolong_levelset_batch: Context.prolong_levelset_to for n pairs (any mix of shapes and channel counts) with one launch."""
    coarses, fines = _pairs(coarses, fines)
    _batch_chk(lib().cvh_prolong_levelset_batch(_member_array(coarses), _member_array(fines), len(coarses)))


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
    contexts = list(contexts)
    _batch_chk(lib().cvh_convert_colour_batch(_member_array(contexts), len(contexts), space, order, int(bool(inverse))))


def luma_image_batch(srcs, dsts, order="bgr"):
    """cvh_luma_image_batch: Context.luma_to for n pairs (any mix of shapes) with one launch."""
    order = order_code(order)
    srcs, dsts = _pairs(srcs, dsts)
    _batch_chk(lib().cvh_luma_image_batch(_member_array(srcs), _member_array(dsts), len(srcs), order))


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
    _batch_chk(call(_member_array(srcs), _member_array(dsts), n, (C.c_int * max(n, 1))(*radii), (C.c_int * max(3 * n, 1))(*flat)))


def local_planes_batch(srcs, dsts, radius, what):
    """cvh_local_planes_batch: Context.local_planes_to for n pairs (any mix of shapes, channel counts, radii and codes) with one set of
    launches.  A scalar `radius` and ONE `what` (a name or a tuple of codes) go to every pair; else one per pair."""
    _window_planes_batch("local", srcs, dsts, radius, what)


def rank_planes_batch(srcs, dsts, radius, what):
    """cvh_rank_planes_batch: Context.rank_planes_to for n pairs (any mix of shapes, channel counts, radii and codes) with one set of
    launches.  A scalar `radius` and ONE `what` (a name or a tuple of codes) go to every pair; else one per pair.  A median's radius
    limit is checked against the codes a destination has planes for."""
    _window_planes_batch("rank", srcs, dsts, radius, what)


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
    contexts = list(contexts)
    n = len(contexts)
    out = (EnergyTerms * max(n, 1))()
    _batch_chk(lib().cvh_energy_batch(_member_array(contexts), n, out))
    return [_energy_of(out[i], contexts[i].channels) for i in range(n)]


def score_batch(contexts, truths, invert=False, tol=2.0, stream=0):
    """cvh_score_mask_device_batch: Context.score for n contexts (any mix of shapes and channel counts) against n truth planes in device
    memory (integer addresses of h * w bytes, non-zero = foreground), with one set of launches and one host wait.  Returns [Score] per
    context; every integer is the member's own Context.score()."""
    contexts, truths = list(contexts), [int(t) or None for t in truths]
    n = len(contexts)
    if len(truths) != n:
        raise ValueError(f"{n} contexts but {len(truths)} truth planes")
    out = (MaskScore * max(n, 1))()
    ptrs = (C.c_void_p * max(n, 1))(*truths)
    _batch_chk(lib().cvh_score_mask_device_batch(_member_array(contexts), n, ptrs, int(bool(invert)), score_tol2(tol), out, int(stream) or None))
    return [_score_of(out[i]) for i in range(n)]


def _clean_args(conn, invert, min_area, fill_holes, keep_largest):
    return int(conn), int(bool(invert)), int(min_area), int(fill_holes), int(keep_largest)


def _r2_array(r2, radius, n):
    """one squared radius per member: r2 / radius are one number for all members or one per member"""
    def per_member(v):
        vals = list(v) if np.ndim(v) else [v] * n
        if len(vals) != n:
            raise ValueError(f"{len(vals)} radii for {n} members")
        return vals
    if r2 is not None and radius is not None:
        raise ValueError("give r2 or radius, not both")
    vals = [_morph_r2(None, float(v)) for v in per_member(radius)] if radius is not None else [_morph_r2(v, None) for v in per_member(0 if r2 is None else r2)]
    return (C.c_uint32 * max(n, 1))(*vals)


def mask_morph_batch(contexts, ptrs, op, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, stream=0):
    """cvh_get_mask_morph_device_batch: Context.mask_morph for n contexts (any mix of shapes and channel counts) into device memory (ptrs:
    one integer address of h * w bytes per context), one set of launches for all; r2 / radius are one number or one per member, op is
    shared.  Work enqueued on `stream` afterwards sees the masks.  Does not block the host."""
    contexts = list(contexts)
    n = len(contexts)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (morph_code(op), _r2_array(r2, radius, n))
    _batch_chk(lib().cvh_get_mask_morph_device_batch(_member_array(contexts), n, _address_array(list(ptrs), n), *args, int(stream) or None))


def morph_levelset_batch(contexts, op, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, inside=1.0,
                         outside=-1.0):
    """cvh_morph_levelset_batch: Context.morph_levelset for n contexts with one set of launches; r2 / radius as in mask_morph_batch."""
    contexts = list(contexts)
    n = len(contexts)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (morph_code(op), _r2_array(r2, radius, n))
    _batch_chk(lib().cvh_morph_levelset_batch(_member_array(contexts), n, *args, float(inside), float(outside)))


def split_geometry():
    """cvh_split_geometry: (tile_rows, tile_cols, group) -- the tile of the growth's sweeps and the sweeps enqueued per host wait."""
    tr, tc, g = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().cvh_split_geometry(C.byref(tr), C.byref(tc), C.byref(g))
    return tr.value, tc.value, g.value


def split_batch(contexts, ptrs=None, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, stream=0):
    """cvh_split_batch: Context.split for n contexts (any mix of shapes and channel counts) with one set of launches.  ptrs: one integer
    device address of h * w int32 labels per context (0 = no label plane for that member), or None; r2 / radius are one number or one per
    member.  Returns [K] per context."""
    contexts = list(contexts)
    n = len(contexts)
    counts = (C.c_int * max(n, 1))()
    addr = None if ptrs is None else _address_array(list(ptrs), n)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (_r2_array(r2, radius, n),)
    _batch_chk(lib().cvh_split_batch(_member_array(contexts), n, *args, addr, counts, int(stream) or None))
    return [counts[i] for i in range(n)]


def split_levelset_batch(contexts, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, inside=1.0,
                         outside=-1.0):
    """cvh_split_levelset_batch: Context.split_levelset for n contexts with one set of launches; r2 / radius as in split_batch."""
    contexts = list(contexts)
    n = len(contexts)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (_r2_array(r2, radius, n),)
    _batch_chk(lib().cvh_split_levelset_batch(_member_array(contexts), n, *args, float(inside), float(outside)))


def init_mask_batch(contexts, ptrs, inside=1.0, outside=-1.0, stream=0):
    """cvh_init_mask_device_batch: Context.init_mask for n contexts from byte masks in device memory (ptrs: one integer address of h * w
    bytes per context, read behind what `stream` holds), one launch for all."""
    contexts = list(contexts)
    n = len(contexts)
    _batch_chk(lib().cvh_init_mask_device_batch(_member_array(contexts), n, _address_array(list(ptrs), n), float(inside), float(outside),
                                                int(stream) or None))


def measure_batch(contexts, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, cap=None, stream=0):
    """cvh_measure_batch: Context.measure for n contexts (any mix of shapes and channel counts) with one set of launches.  cap: None
    (all rows, at the price of a first call for the counts), one number for every member or one per member.  Returns [(K, table)] per
    context; every row is bit for bit the member's own Context.measure()."""
    contexts = list(contexts)
    n = len(contexts)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest)
    counts = (C.c_int * max(n, 1))()
    if cap is None:
        _batch_chk(lib().cvh_measure_batch(_member_array(contexts), n, *args, None, None, counts, int(stream) or None))
        caps = [counts[i] for i in range(n)]
    else:
        caps = [int(c) for c in cap] if np.ndim(cap) else [int(cap)] * n
        if len(caps) != n:
            raise ValueError(f"cap: {len(caps)} values for {n} members")
    tables = [np.zeros(max(c, 0), dtype=REGION_DTYPE) for c in caps]
    if any(t.size for t in tables) or cap is not None:
        ptrs = (C.c_void_p * max(n, 1))(*[t.ctypes.data if t.size else None for t in tables])
        _batch_chk(lib().cvh_measure_batch(_member_array(contexts), n, *args, ptrs, (C.c_int * max(n, 1))(*caps), counts, int(stream) or None))
    return [(counts[i], tables[i][:min(counts[i], tables[i].size)].copy()) for i in range(n)]


def overlaps_batch(contexts, others, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, cap=None, stream=0):
    """cvh_overlaps_device_batch: Context.overlaps for n contexts (any mix of shapes and channel counts) against n int32 label planes in
    device memory (integer addresses of h * w int32), with one set of launches.  cap: None (all rows, at the price of a first call for
    the counts), one number for every member or one per member.  Returns [(rows, K)] per context; every row is byte for byte the
    member's own Context.overlaps()."""
    contexts = list(contexts)
    n = len(contexts)
    args = _clean_args(conn, invert, min_area, fill_holes, keep_largest)
    longs = C.c_long * max(n, 1)
    pairs, counts = longs(), (C.c_int * max(n, 1))()
    ptrs = _address_array(list(others), n)
    if cap is None:
        _batch_chk(lib().cvh_overlaps_device_batch(_member_array(contexts), n, *args, ptrs, None, None, pairs, counts, int(stream) or None))
        caps = [pairs[i] for i in range(n)]
    else:
        caps = [int(c) for c in cap] if np.ndim(cap) else [int(cap)] * n
        if len(caps) != n:
            raise ValueError(f"cap: {len(caps)} values for {n} members")
    tables = [np.zeros(max(c, 0), dtype=OVERLAP_DTYPE) for c in caps]
    tptrs = (C.c_void_p * max(n, 1))(*[t.ctypes.data if t.size else None for t in tables])
    _batch_chk(lib().cvh_overlaps_device_batch(_member_array(contexts), n, *args, ptrs, tptrs, longs(*caps), pairs, counts, int(stream) or None))
    return [(tables[i][:min(pairs[i], tables[i].size)].copy(), counts[i]) for i in range(n)]


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
    contexts = list(contexts)
    n = len(contexts)
    longs = C.c_long * max(n, 1)
    nloops, npoints = longs(), longs()
    if loop_caps is None:
        _batch_chk(fn(_member_array(contexts), n, *args, None, None, None, None, nloops, npoints, int(stream) or None))
        loop_caps = [nloops[i] for i in range(n)]
    loop_caps = [int(c) for c in loop_caps]
    if len(loop_caps) != n:
        raise ValueError(f"loop_caps: {len(loop_caps)} values for {n} members")
    tables = [np.zeros(max(c, 0), dtype=CONTOUR_LOOP_DTYPE) for c in loop_caps]
    tptrs = (C.c_void_p * max(n, 1))(*[t.ctypes.data if t.size else None for t in tables])
    pptrs, pcaps = None, None
    if d_points is not None:
        d_points, point_caps = [int(p) or None for p in d_points], [int(c) for c in point_caps]
        if len(d_points) != n or len(point_caps) != n:
            raise ValueError(f"{n} contexts but {len(d_points)} point arrays and {len(point_caps)} caps")
        pptrs, pcaps = (C.c_void_p * max(n, 1))(*d_points), longs(*point_caps)
    _batch_chk(fn(_member_array(contexts), n, *args, tptrs, longs(*loop_caps), pptrs, pcaps, nloops, npoints, int(stream) or None))
    return [(nloops[i], npoints[i], tables[i][:min(nloops[i], tables[i].size)].copy()) for i in range(n)]


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


def multiphase_run(a, b, max_steps=-1, trace=False):
    """cvh_multiphase_run ("Four phases" in include/chanvese_hip.h): contexts a and b hold phi1 and phi2 of a Vese-Chan pair and are
    iterated together until max_steps iterations are done (negative: no bound) or the pair stops.  Returns (steps_done, (norm1, norm2),
    trace): trace is None, or with trace=True (all rows; needs max_steps >= 0) or trace=<rows> an array of one row of 4 C + 2 doubles
    per iteration -- the means c11, c10, c01, c00 it used and its two norms.  Both contexts are left as set_levelset of the new level
    sets leaves them."""
    want = 0 if trace is False or trace is None else (int(max_steps) if trace is True else int(trace))
    if want < 0:
        raise ValueError("trace=True needs max_steps >= 0 (or pass the number of rows)")
    done, rows, norms = C.c_int(0), C.c_int(0), (C.c_double * 2)()
    out = np.zeros((max(want, 1), 4 * a.channels + 2), dtype=np.float64) if want or trace is True else None
    _batch_chk(lib().cvh_multiphase_run(a._h, b._h, int(max_steps), C.byref(done), norms, None if out is None else _dp(out), want, C.byref(rows)))
    return done.value, (norms[0], norms[1]), None if out is None else out[:rows.value].copy()


def _trace_rows_wanted(max_steps, trace):
    want = 0 if trace is False or trace is None else (int(max_steps) if trace is True else int(trace))
    if want < 0:
        raise ValueError("trace=True needs max_steps >= 0 (or pass the number of rows)")
    return want


def multiphase_run_batch(pairs, max_steps=-1, trace=False):
    """cvh_multiphase_run_batch: multiphase_run for every pair (a, b) of `pairs` at once -- per iteration one step launch and one
    finalise launch for all pairs of a (channel count, math mode) class.  Every pair iterates and stops on its own and is bit for bit
    what multiphase_run gives for it alone.  Returns a list of (steps_done, (norm1, norm2), trace), one per pair; trace as there."""
    pairs = [tuple(p) for p in pairs]
    n = len(pairs)
    if n == 0:
        raise ValueError("multiphase_run_batch: no pairs")
    if any(len(p) != 2 for p in pairs):
        raise ValueError("multiphase_run_batch: every member is a pair (a, b) of contexts")
    want = _trace_rows_wanted(max_steps, trace)
    wanted = bool(want) or trace is True
    done, rows, norms = (C.c_int * n)(), (C.c_int * n)(), (C.c_double * (2 * n))()
    outs = [np.zeros((max(want, 1), 4 * a.channels + 2), dtype=np.float64) for a, _ in pairs] if wanted else None
    traces = (C.c_void_p * n)(*[o.ctypes.data for o in outs]) if wanted else None
    _batch_chk(lib().cvh_multiphase_run_batch(_member_array([a for a, _ in pairs]), _member_array([b for _, b in pairs]), n, int(max_steps), done, norms,
                                              traces, want, rows))
    return [(done[i], (norms[2 * i], norms[2 * i + 1]), outs[i][:rows[i]].copy() if wanted else None) for i in range(n)]


def multiphase_means(a, b):
    """cvh_multiphase_means: the means of the current pair as an array of (4, C), rows c11, c10, c01, c00.  Only reads."""
    c = np.zeros((4, a.channels), dtype=np.float64)
    _batch_chk(lib().cvh_multiphase_means(a._h, b._h, _dp(c)))
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
    want = 0 if trace is False or trace is None else (int(max_steps) if trace is True else int(trace))
    if want < 0:
        raise ValueError("trace=True needs max_steps >= 0 (or pass the number of rows)")
    done, rows, norm = C.c_int(0), C.c_int(0), C.c_double(0.0)
    out = np.zeros(max(want, 1), dtype=np.float64) if want or trace is True else None
    ctx._chk(lib().cvh_localized_run(ctx._h, int(radius), int(max_steps), C.byref(done), C.byref(norm), None if out is None else _dp(out), want,
                                     C.byref(rows)))
    return done.value, norm.value, None if out is None else out[:rows.value].copy()


def localized_run_batch(contexts, radius, max_steps=-1, trace=False):
    """cvh_localized_run_batch: localized_run for every context at once -- per iteration one row-pass, one step and one finalise launch
    for all members of a (channel count, math mode) class.  radius is an int (the same for every member) or a sequence of one value per
    member.  Every member iterates and stops on its own and is bit for bit what localized_run gives for it alone.  Returns a list of
    (steps_done, norm, trace), one per member; trace as there."""
    contexts = list(contexts)
    n = len(contexts)
    if n == 0:
        raise ValueError("localized_run_batch: no members")
    radii = [int(r) for r in radius] if np.ndim(radius) else [int(radius)] * n
    if len(radii) != n:
        raise ValueError(f"radius: {len(radii)} values for {n} members")
    want = _trace_rows_wanted(max_steps, trace)
    wanted = bool(want) or trace is True
    done, rows, norms = (C.c_int * n)(), (C.c_int * n)(), (C.c_double * n)()
    outs = [np.zeros(max(want, 1), dtype=np.float64) for _ in contexts] if wanted else None
    traces = (C.c_void_p * n)(*[o.ctypes.data for o in outs]) if wanted else None
    _batch_chk(lib().cvh_localized_run_batch(_member_array(contexts), n, (C.c_int * n)(*radii), int(max_steps), done, norms, traces, want, rows))
    return [(done[i], norms[i], outs[i][:rows[i]].copy() if wanted else None) for i in range(n)]


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
    ks = [float(k) for k in K] if np.ndim(K) else [float(K)] * n
    if len(ks) != n:
        raise ValueError(f"K: {len(ks)} values for {n} pairs")
    _batch_chk(lib().cvh_edge_map_batch(_member_array(dsts), _member_array(srcs), n, (C.c_double * n)(*ks)))


def geodesic_run(ctx, max_steps=-1, trace=False):
    """cvh_geodesic_run ("Edge-weighted length" in include/chanvese_hip.h): Chan-Vese with the length term weighted by the context's
    edge plane, until max_steps iterations are done (negative: no bound) or the stop rule fires.  Returns (steps_done, norm, trace):
    trace is None, or with trace=True (all rows; needs max_steps >= 0) or trace=<rows> an array of one row of 2 C + 1 doubles per
    iteration -- the means c1, c2 it used and its norm.  The context is left as set_levelset of the new level set leaves it."""
    want = _trace_rows_wanted(max_steps, trace)
    done, rows, norm = C.c_int(0), C.c_int(0), C.c_double(0.0)
    out = np.zeros((max(want, 1), 2 * ctx.channels + 1), dtype=np.float64) if want or trace is True else None
    ctx._chk(lib().cvh_geodesic_run(ctx._h, int(max_steps), C.byref(done), C.byref(norm), None if out is None else _dp(out), want, C.byref(rows)))
    return done.value, norm.value, None if out is None else out[:rows.value].copy()


def geodesic_run_batch(contexts, max_steps=-1, trace=False):
    """cvh_geodesic_run_batch: geodesic_run for every context at once -- per iteration one step and one finalise launch for all members
    of a (channel count, math mode) class.  Every member iterates and stops on its own and is bit for bit what geodesic_run gives for
    it alone.  Returns a list of (steps_done, norm, trace), one per member; trace as there."""
    contexts = list(contexts)
    n = len(contexts)
    if n == 0:
        raise ValueError("geodesic_run_batch: no members")
    want = _trace_rows_wanted(max_steps, trace)
    wanted = bool(want) or trace is True
    done, rows, norms = (C.c_int * n)(), (C.c_int * n)(), (C.c_double * n)()
    outs = [np.zeros((max(want, 1), 2 * c.channels + 1), dtype=np.float64) for c in contexts] if wanted else None
    traces = (C.c_void_p * n)(*[o.ctypes.data for o in outs]) if wanted else None
    _batch_chk(lib().cvh_geodesic_run_batch(_member_array(contexts), n, int(max_steps), done, norms, traces, want, rows))
    return [(done[i], norms[i], outs[i][:rows[i]].copy() if wanted else None) for i in range(n)]


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
            raise CvhError(rc, self._L.cvh_last_error(None).decode())

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
        self._chk(self._L.cvh_set_image_device(self._h, int(ptr) or None, int(layout), int(stream) or None))

    def get_image_device(self, ptr, layout=LAYOUT_PLANAR, stream=0):
        self._chk(self._L.cvh_get_image_device(self._h, int(ptr) or None, int(layout), int(stream) or None))

    def set_levelset_device(self, ptr, bits=64, stream=0):
        self._chk(self._L.cvh_set_levelset_device(self._h, int(ptr) or None, int(bits), int(stream) or None))

    def get_levelset_device(self, ptr, bits=64, stream=0):
        self._chk(self._L.cvh_get_levelset_device(self._h, int(ptr) or None, int(bits), int(stream) or None))

    def get_mask_device(self, ptr, invert=False, stream=0):
        self._chk(self._L.cvh_get_mask_device(self._h, int(ptr) or None, int(bool(invert)), int(stream) or None))

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
        _batch_chk(self._L.cvh_restrict_image(self._h, coarse._h))

    def prolong_levelset_to(self, fine):
        """cvh_prolong_levelset: the level set of this context, replicated 2 x 2 bit for bit, becomes the level set of `fine`, exactly
        as its set_levelset of those doubles (a new run begins there); this context is only read."""
        _batch_chk(self._L.cvh_prolong_levelset(self._h, fine._h))

    def convert_colour(self, space, order="bgr", inverse=False):
        """cvh_convert_colour: the three planes, read as (B, G, R) or (R, G, B) by `order`, become (Y, Cr, Cb) ("ycrcb") or (Y, U, V)
        ("yuv") in place on the device -- or, with inverse, back --, exactly as set_image of the converted bytes (the header's integer
        definition).  The library does not remember which space the planes are in."""
        space, order = colour_space_code(space), order_code(order)
        _batch_chk(self._L.cvh_convert_colour(self._h, space, order, int(bool(inverse))))

    def luma_to(self, dst, order="bgr"):
        """cvh_luma_image: the Y of this three-channel context becomes the image of `dst` (a one-channel context of the same shape),
        exactly as its set_image of that plane; this context is only read."""
        order = order_code(order)
        _batch_chk(self._L.cvh_luma_image(self._h, dst._h, order))

    def _window_planes_to(self, family, dst, radius, what):
        radii, codes = _window_args(family, [radius], [what], [dst])   # (checked before the library is reached)
        _batch_chk(getattr(self._L, f"cvh_{family}_planes")(self._h, dst._h, radii[0], (C.c_int * 3)(*codes[0])))

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
        _batch_chk(self._L.cvh_energy(self._h, C.byref(t)))
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
            _batch_chk(self._L.cvh_score_mask(self._h, _u8p(t), int(bool(invert)), tol2, C.byref(s)))
        else:
            _batch_chk(self._L.cvh_score_mask_device(self._h, int(truth) or None, int(bool(invert)), tol2, C.byref(s), int(stream) or None))
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
            self._chk(self._L.cvh_set_edge_map_device(self._h, int(gq) or None, int(stream) or None))
        else:
            raise ValueError(f"set_edge_map: a uint16 numpy array or the integer address of device memory, got {type(gq).__name__}")

    def get_edge_map(self, ptr=0, stream=0):
        """cvh_get_edge_map / cvh_get_edge_map_device: the edge plane as a uint16 array of (h, w), or written to device memory at `ptr`."""
        if ptr:
            self._chk(self._L.cvh_get_edge_map_device(self._h, int(ptr), int(stream) or None))
            return None
        out = np.empty((self.h, self.w), dtype=np.uint16)
        self._chk(self._L.cvh_get_edge_map(self._h, out.ctypes.data))
        return out

    def edge_map_from(self, src, K):
        """cvh_edge_map: this context's edge plane from the planes of `src` (may be self) as they are now:
        gq = rint(32768 / (1 + |Sobel gradient|^2 / (64 C K^2))).  Smooth first (perona_malik, or a local mean in a second context)."""
        _batch_chk(self._L.cvh_edge_map(self._h, src._h, float(K)))

    def multiphase_labels_with(self, b, ptr=0, stream=0):
        """cvh_multiphase_labels / _device: label = mask(self) + 2 mask(b) per pixel, one launch.  Returns a uint8 array of (h, w), or
        with ptr (an integer device address of h * w bytes, ordered behind `stream`) writes there without a host wait.  Only reads."""
        if ptr:
            _batch_chk(self._L.cvh_multiphase_labels_device(self._h, b._h, int(ptr), int(stream) or None))
            return None
        out = np.empty((self.h, self.w), dtype=np.uint8)
        _batch_chk(self._L.cvh_multiphase_labels(self._h, b._h, _u8p(out)))
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
        args = (int(conn), int(bool(invert)))
        if cap is None:
            self._chk(self._L.cvh_components(self._h, *args, int(labels_ptr) or None, None, 0, C.byref(count), int(stream) or None))
            table = np.zeros(count.value, dtype=COMPONENT_DTYPE)
            if count.value:
                self._chk(self._L.cvh_components(self._h, *args, None, table.ctypes.data, count.value, C.byref(count), None))
            return count.value, table
        table = np.zeros(max(int(cap), 0), dtype=COMPONENT_DTYPE)
        self._chk(self._L.cvh_components(self._h, *args, int(labels_ptr) or None, table.ctypes.data if table.size else None, int(cap),
                                         C.byref(count), int(stream) or None))
        return count.value, table[:min(count.value, table.size)].copy()

    def measure(self, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, cap=None, stream=0):
        """cvh_measure: the components of the mask -- get_mask_clean's for the same five options, (0, 0, False) the raw one -- measured
        on the device.  Returns (K, table): table is a structured array (REGION_DTYPE) of the first min(K, cap) rows: first, area, box,
        border, perimeter, coordinate sums and the sums of the image planes and their squares (region_shapes derives centroid, moments,
        axes, mean and variance).  cap = None asks for all K rows and COSTS TWO LABELLINGS (as components); pass a cap where an upper
        bound of K is known, cap = 0 for the count alone.  Only reads: a run continued after it is bit-identical to one without."""
        count = C.c_int(0)
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest)
        if cap is None:
            _batch_chk(self._L.cvh_measure(self._h, *args, None, 0, C.byref(count), int(stream) or None))
            if not count.value:
                return 0, np.zeros(0, dtype=REGION_DTYPE)
            cap = count.value
        table = np.zeros(max(int(cap), 0), dtype=REGION_DTYPE)
        _batch_chk(self._L.cvh_measure(self._h, *args, table.ctypes.data if table.size else None, int(cap), C.byref(count), int(stream) or None))
        return count.value, table[:min(count.value, table.size)].copy()

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
                _batch_chk(self._L.cvh_overlaps(self._h, *args, plane.ctypes.data, table, cap_, C.byref(pairs), C.byref(count)))
        else:
            def call(table, cap_):
                _batch_chk(self._L.cvh_overlaps_device(self._h, *args, int(other) or None, table, cap_, C.byref(pairs), C.byref(count),
                                                       int(stream) or None))
        if cap is None:
            call(None, 0)
            cap = pairs.value
        table = np.zeros(max(int(cap), 0), dtype=OVERLAP_DTYPE)
        call(table.ctypes.data if table.size else None, int(cap))
        return table[:min(pairs.value, table.size)].copy(), count.value

    def contour_counts(self, conn=8, invert=False, min_area=0, fill_holes=0, keep_largest=False, simplify=True):
        """cvh_contours without outputs: (nloops, npoints) of the boundary of the mask."""
        nloops, npoints = C.c_long(0), C.c_long(0)
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (int(bool(simplify)),)
        _batch_chk(self._L.cvh_contours(self._h, *args, None, 0, None, 0, C.byref(nloops), C.byref(npoints)))
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
            _batch_chk(self._L.cvh_contours(self._h, *args, loops.ctypes.data, nl, points.ctypes.data, npts, C.byref(nloops), C.byref(npoints)))
        return loops, points

    def contours_subpixel(self, conn=8, invert=False, min_area=0, fill_holes=0, keep_largest=False):
        """cvh_contours_subpixel: the zero level of the level set as ordered closed polygons -- the loops of contours(simplify=False) for
        the same five options, each lattice point replaced by the point where u changes sign across that edge (the edge's midpoint
        where it does not: the plane's border, a pixel cleaning reclassified, NaN, zeros, infinities).  Returns (loops, points): loops
        as contours() gives them with simplify=False, points a float64 array (P, 2) of x, y with pixel centres at half-integers.
        COSTS TWO TRACES (the counts size the arrays).  Only reads: a run continued after it is bit-identical to one without."""
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest)
        nloops, npoints = C.c_long(0), C.c_long(0)
        _batch_chk(self._L.cvh_contours_subpixel(self._h, *args, None, 0, None, 0, C.byref(nloops), C.byref(npoints)))
        nl, npts = nloops.value, npoints.value
        loops, points = np.zeros(nl, dtype=CONTOUR_LOOP_DTYPE), np.zeros((npts, 2), dtype=np.float64)
        if nl:
            _batch_chk(self._L.cvh_contours_subpixel(self._h, *args, loops.ctypes.data, nl, points.ctypes.data, npts, C.byref(nloops), C.byref(npoints)))
        return loops, points

    def get_mask_clean(self, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False):
        """cvh_get_mask_clean: the mask without foreground components below min_area, with the holes of area <= fill_holes filled
        (-1: any size) and, with keep_largest, only its largest component; (0, 0, False) is get_mask."""
        m = np.empty((self.h, self.w), dtype=np.uint8)
        self._chk(self._L.cvh_get_mask_clean(self._h, _u8p(m), int(conn), int(bool(invert)), int(min_area), int(fill_holes), int(keep_largest)))
        return m

    def get_mask_clean_device(self, ptr, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, stream=0):
        self._chk(self._L.cvh_get_mask_clean_device(self._h, int(ptr) or None, int(conn), int(bool(invert)), int(min_area), int(fill_holes),
                                                    int(keep_largest), int(stream) or None))

    def mask_morph(self, op, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, out=None, stream=0):
        """cvh_get_mask_morph / cvh_get_mask_morph_device: the cleaned mask (get_mask_clean's arguments) dilated, eroded, opened or closed
        by the disk dx^2 + dy^2 <= r2 (or radius: r2 = floor(radius^2)) on the device; op is a MORPH_* code or its name.  out is None (a
        new (h, w) uint8 array is returned), a contiguous uint8 array of (h, w) to fill, or the integer address of h * w bytes in device
        memory, written behind what `stream` holds.  Only reads: a run continued after it is bit-identical to one without."""
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (morph_code(op), _morph_r2(r2, radius))
        if out is None or isinstance(out, np.ndarray):
            m = np.empty((self.h, self.w), dtype=np.uint8) if out is None else out
            assert m.dtype == np.uint8 and m.shape == (self.h, self.w) and m.flags["C_CONTIGUOUS"]
            _batch_chk(self._L.cvh_get_mask_morph(self._h, _u8p(m), *args))
            return m
        _batch_chk(self._L.cvh_get_mask_morph_device(self._h, int(out) or None, *args, int(stream) or None))
        return out

    def split(self, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, labels_ptr=0, cap=None, stream=0):
        """cvh_split: the cleaned mask (get_mask_clean's arguments) taken apart into one object per core of its erosion by the disk
        dx^2 + dy^2 <= r2 (r2, or radius with r2 = floor(radius^2)): "Object split" in include/chanvese_hip.h.  labels_ptr: integer device
        address of h * w int32 (0 = no label plane).  Returns (labels, table, K): labels is labels_ptr or None; table is a structured array
        (COMPONENT_DTYPE) of the first min(K, cap) rows -- `first` the marker's smallest flat index, area and box those of the grown
        object.  cap = None asks for all K rows and COSTS TWO CALLS (as components); cap = 0 for no table.  Only reads."""
        count = C.c_int(0)
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (_morph_r2(r2, radius),)
        labels = int(labels_ptr) or None
        if cap is None:
            _batch_chk(self._L.cvh_split(self._h, *args, labels, None, 0, C.byref(count), int(stream) or None))
            table = np.zeros(count.value, dtype=COMPONENT_DTYPE)
            if count.value:
                _batch_chk(self._L.cvh_split(self._h, *args, None, table.ctypes.data, count.value, C.byref(count), None))
            return labels, table, count.value
        table = np.zeros(max(int(cap), 0), dtype=COMPONENT_DTYPE)
        _batch_chk(self._L.cvh_split(self._h, *args, labels, table.ctypes.data if table.size else None, int(cap), C.byref(count), int(stream) or None))
        return labels, table[:min(count.value, table.size)].copy(), count.value

    def split_labels(self, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False):
        """cvh_split_host: split()'s label plane as a numpy int32 array (h, w) in host memory, and K: (labels, K)."""
        count = C.c_int(0)
        labels = np.empty((self.h, self.w), dtype=np.int32)
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (_morph_r2(r2, radius),)
        _batch_chk(self._L.cvh_split_host(self._h, *args, labels.ctypes.data, None, 0, C.byref(count)))
        return labels, count.value

    def split_levelset(self, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, inside=1.0, outside=-1.0):
        """cvh_split_levelset: split in place -- the level set becomes `inside` on the split objects and `outside` on the cut lines and the
        background, and a new run begins; components, measure, contours, overlaps and further iterations then see the split objects."""
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (_morph_r2(r2, radius),)
        _batch_chk(self._L.cvh_split_levelset(self._h, *args, float(inside), float(outside)))

    def morph_levelset(self, op, r2=None, radius=None, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, inside=1.0,
                       outside=-1.0):
        """cvh_morph_levelset: mask_morph in place -- the level set becomes `inside` where that mask is 1 and `outside` elsewhere, and a
        new run begins as after set_levelset; the mask never leaves the device.  With MORPH_NONE the cleaned mask is baked in."""
        args = _clean_args(conn, invert, min_area, fill_holes, keep_largest) + (morph_code(op), _morph_r2(r2, radius))
        _batch_chk(self._L.cvh_morph_levelset(self._h, *args, float(inside), float(outside)))

    def init_mask(self, mask, inside=1.0, outside=-1.0, stream=0):
        """cvh_init_mask / cvh_init_mask_device: u = inside where the mask's byte is nonzero, outside elsewhere, written on the device (one
        byte per pixel crosses, not eight); the context is left as set_levelset of those doubles leaves it.  mask is a numpy array of
        (h, w), bool or uint8, or the integer address of h * w bytes in device memory, read behind what `stream` holds.  Needs neither
        an image nor a level set."""
        if isinstance(mask, np.ndarray):
            m = np.ascontiguousarray(mask.view(np.uint8) if mask.dtype == np.bool_ else mask, dtype=np.uint8)
            assert m.shape == (self.h, self.w)
            _batch_chk(self._L.cvh_init_mask(self._h, _u8p(m), float(inside), float(outside)))
        else:
            _batch_chk(self._L.cvh_init_mask_device(self._h, int(mask) or None, float(inside), float(outside), int(stream) or None))

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
