"""What mirrors include/chanvese_hip.h on the Python side: the constants, the structs, the numpy dtypes of the table rows, the loaded
library and the one table of its signatures.  capi.py imports these names and is the public namespace; nothing here marshals a call."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CHANVESE_HIP_LIB selects another BUILD of the same library (A/B variants under csrc/variants/, tools/build_variant.sh)
LIB_PATH = os.environ.get("CHANVESE_HIP_LIB") or os.path.join(_HERE, "csrc", "libchanvese_hip.so")

CVH_OK = 0
OP_DELTA, OP_HEAVISIDE, OP_ONE_MINUS_HEAVISIDE = 0, 1, 2
MATH_DEFAULT, MATH_STRICT, MATH_FAST = 0, 1, 2

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
# "Smoothing": what plane k of the destination of cvh_smooth_planes becomes, by code and -- every plane alike -- by name
SMOOTH_COPY, SMOOTH_BLUR, SMOOTH_DETAIL = 0, 1, 2
SMOOTH_RADIUS_MAX, SMOOTH_TAP_SUM = 63, 32768
SMOOTH_WHATS = {"blur": SMOOTH_BLUR, "detail": SMOOTH_DETAIL}


class Params(C.Structure):
    """struct cvh_params (src/main.cpp:731-734 of the reference)."""
    _fields_ = [("mu", C.c_double), ("nu", C.c_double), ("dt", C.c_double),
                ("eps", C.c_double), ("tol", C.c_double),
                ("lambda1", C.c_double * 3), ("lambda2", C.c_double * 3)]


class EnergyTerms(C.Structure):
    """struct cvh_energy_terms ("Energy" in include/chanvese_hip.h)."""
    _fields_ = [("total", C.c_double), ("length", C.c_double), ("area", C.c_double),
                ("fit_in", C.c_double * 3), ("fit_out", C.c_double * 3), ("c1", C.c_double * 3), ("c2", C.c_double * 3)]


class MaskScore(C.Structure):
    """struct cvh_mask_score ("Mask scores" in include/chanvese_hip.h)."""
    _fields_ = [(f, C.c_uint64) for f in ("tp", "fp", "fn", "tn", "surf_m", "surf_t", "within_m", "within_t", "dist_m_q16", "dist_t_q16")] + \
               [("hd2_m", C.c_uint32), ("hd2_t", C.c_uint32), ("defined", C.c_int32), ("pad", C.c_int32)]


class ConvexParams(C.Structure):
    """struct cvh_convex_params ("Convex relaxation" in include/chanvese_hip.h)."""
    _fields_ = [("tau", C.c_double), ("sigma", C.c_double), ("stop_rms", C.c_double),
                ("means_every", C.c_int), ("use_edge", C.c_int), ("resume", C.c_int)]


class Match(C.Structure):
    """struct cvh_match ("Component overlaps" in include/chanvese_hip.h)."""
    _fields_ = [(f, C.c_uint32) for f in ("objects_a", "objects_b", "tp", "fp", "fn", "pad")]


class CvhError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"chanvese_hip error {code}: {msg}")
        self.code = code


# ---- the signatures: every symbol include/chanvese_hip.h declares, once
_int, _long, _dbl, _u32, _vp = C.c_int, C.c_long, C.c_double, C.c_uint32, C.c_void_p
_ip, _lp, _dp, _fp, _u8p, _u32p = (C.POINTER(t) for t in (_int, _long, _dbl, C.c_float, C.c_uint8, _u32))
_u8pp, _vpp = C.POINTER(_u8p), C.POINTER(_vp)
_u16p = C.POINTER(C.c_uint16)
# the argument groups that recur (a context, a device address, a host table and a stream are all void *)
MEMBERS = [_vpp, _int]                        # member list + n
MARCH_MEMBERS = [_vp, _int]                   # the same of the march batches, which declare their lists void *
PAIRS = [_vpp, _vpp, _int]                    # two member lists of n pairs + n
MASK = [_int, _int, _long, _long, _int]       # the mask options: conn, invert, min_area, fill_holes, keep_largest
TABLE = [_vp, _int, _ip]                      # table, cap, count
TABLES = [_vpp, _ip, _ip]                     # one table per member, caps, counts
OVERLAPS = [_vp, _long, _lp, _ip]             # table, cap, pairs, count
LOOPS = [_vp, _long, _vp, _long, _lp, _lp]    # loops, loop_cap, points, point_cap, nloops, npoints
LOOPS_BATCH = [_vpp, _lp, _vpp, _lp, _lp, _lp]
FILL = [_dbl, _dbl]                           # inside, outside
RUN = [_int, _ip, _dp]                        # max_steps, steps_done, norm(s)
TRACE = [_int, _ip]                           # trace_rows, rows


def _sig(*args, res=_int):
    """(restype, argtypes): every argument a ctypes type or one of the groups above"""
    return res, [t for a in args for t in (a if isinstance(a, list) else [a])]


SIGNATURES = {
    "cvh_default_params": _sig(C.POINTER(Params), res=None),
    "cvh_device_count": _sig(_ip),
    "cvh_create": _sig(_vpp, _int, _int, _int, C.POINTER(Params), _int),
    "cvh_destroy": _sig(_vp, res=None),
    "cvh_last_error": _sig(_vp, res=C.c_char_p),
    "cvh_set_params": _sig(_vp, C.POINTER(Params)),
    "cvh_set_option": _sig(_vp, C.c_char_p, _long),
    "cvh_set_image": _sig(_vp, _u8pp),
    "cvh_get_image": _sig(_vp, _u8pp),
    "cvh_set_levelset": _sig(_vp, _dp),
    "cvh_get_levelset": _sig(_vp, _dp),
    "cvh_init_checkerboard": _sig(_vp),
    "cvh_levelset_checkerboard_host": _sig(_int, _int, _dp, res=None),
    "cvh_run": _sig(_vp, RUN),
    "cvh_enqueue_steps": _sig(_vp, _int),
    "cvh_warm": _sig(_vp, _int),
    "cvh_sync": _sig(_vp, _ip, _dp, _ip),
    "cvh_reset_run": _sig(_vp),
    "cvh_get_means": _sig(_vp, _dp, _dp),
    "cvh_get_trace": _sig(_vp, _dp, TRACE),
    "cvh_get_stop_condition": _sig(_vp, _dp),
    "cvh_get_mask": _sig(_vp, _u8p, _int),
    "cvh_get_contour": _sig(_vp, _u8p),
    "cvh_separate": _sig(_vp, _u8p, _int, _u8p),
    "cvh_perona_malik": _sig(_vp, _dbl, _dbl, _dbl),
    "cvh_pm_trip_count": _sig(_dbl, _dbl),
    "cvh_last_run_ms": _sig(_vp, _fp),
    "cvh_last_pm_ms": _sig(_vp, _fp),
    "cvh_ppf_apply": _sig(_dp, _int, _long, _long, _int, _dbl, _int),
    "cvh_ppf_apply_device": _sig(_dp, _long, _int, _dbl, _vp),
    "cvh_version": _sig(res=C.c_char_p),
    "cvh_launch_info": _sig(_vp, _int, C.c_char_p, _int),
    "cvh_enqueue_steps_batch": _sig(MEMBERS, _int),
    "cvh_run_batch": _sig(MEMBERS, RUN),
    "cvh_perona_malik_batch": _sig(MEMBERS, _dp, _dp, _dp),
    "cvh_set_image_device": _sig(_vp, _vp, _int, _vp),
    "cvh_get_image_device": _sig(_vp, _vp, _int, _vp),
    "cvh_set_levelset_device": _sig(_vp, _vp, _int, _vp),
    "cvh_get_levelset_device": _sig(_vp, _vp, _int, _vp),
    "cvh_get_mask_device": _sig(_vp, _vp, _int, _vp),
    "cvh_set_image_device_batch": _sig(MEMBERS, _vpp, _int, _vp),
    "cvh_init_checkerboard_batch": _sig(MEMBERS),
    "cvh_get_mask_device_batch": _sig(MEMBERS, _vpp, _int, _vp),
    "cvh_reinit": _sig(_vp, _ip),
    "cvh_reinit_batch": _sig(MEMBERS, _ip),
    "cvh_components": _sig(_vp, _int, _int, _vp, TABLE, _vp),
    "cvh_components_batch": _sig(MEMBERS, _int, _int, _vpp, _ip, _vp),
    "cvh_get_mask_clean": _sig(_vp, _u8p, MASK),
    "cvh_get_mask_clean_device": _sig(_vp, _vp, MASK, _vp),
    "cvh_get_mask_clean_device_batch": _sig(MEMBERS, _vpp, MASK, _vp),
    "cvh_histogram": _sig(_vp, _vp, _int, _ip),
    "cvh_histogram_batch": _sig(MEMBERS, _vpp, _ip),
    "cvh_otsu_from_histogram": _sig(_vp, _int, _ip),
    "cvh_otsu_threshold": _sig(_vp, _ip),
    "cvh_init_threshold": _sig(_vp, _int, FILL),
    "cvh_init_threshold_batch": _sig(MEMBERS, _ip, FILL),
    "cvh_init_otsu": _sig(_vp, _ip, FILL),
    "cvh_init_otsu_batch": _sig(MEMBERS, _ip, FILL),
    "cvh_init_rect": _sig(_vp, _int, _int, _int, _int, FILL),
    "cvh_init_rect_batch": _sig(MEMBERS, _ip, FILL),
    "cvh_init_disk": _sig(_vp, _int, _int, _int, FILL),
    "cvh_init_disk_batch": _sig(MEMBERS, _ip, FILL),
    "cvh_restrict_image": _sig(_vp, _vp),
    "cvh_restrict_image_batch": _sig(PAIRS),
    "cvh_prolong_levelset": _sig(_vp, _vp),
    "cvh_prolong_levelset_batch": _sig(PAIRS),
    "cvh_convert_colour": _sig(_vp, _int, _int, _int),
    "cvh_convert_colour_batch": _sig(MEMBERS, _int, _int, _int),
    "cvh_luma_image": _sig(_vp, _vp, _int),
    "cvh_luma_image_batch": _sig(PAIRS, _int),
    "cvh_local_planes": _sig(_vp, _vp, _int, _ip),
    "cvh_local_planes_batch": _sig(PAIRS, _ip, _ip),
    "cvh_rank_planes": _sig(_vp, _vp, _int, _ip),
    "cvh_rank_planes_batch": _sig(PAIRS, _ip, _ip),
    "cvh_gauss_taps": _sig(_dbl, _u16p, _ip),
    "cvh_smooth_planes": _sig(_vp, _vp, _int, _u16p, _ip),
    "cvh_smooth_planes_batch": _sig(PAIRS, _ip, C.POINTER(_u16p), _ip),
    "cvh_energy": _sig(_vp, C.POINTER(EnergyTerms)),
    "cvh_energy_batch": _sig(MEMBERS, C.POINTER(EnergyTerms)),
    "cvh_score_mask": _sig(_vp, _u8p, _int, _u32, C.POINTER(MaskScore)),
    "cvh_score_mask_device": _sig(_vp, _vp, _int, _u32, C.POINTER(MaskScore), _vp),
    "cvh_score_mask_device_batch": _sig(MEMBERS, _vpp, _int, _u32, C.POINTER(MaskScore), _vp),
    "cvh_measure": _sig(_vp, MASK, TABLE, _vp),
    "cvh_measure_batch": _sig(MEMBERS, MASK, TABLES, _vp),
    "cvh_region_shape_of": _sig(_vp, _int, _vp),
    "cvh_overlaps": _sig(_vp, MASK, _vp, OVERLAPS),
    "cvh_overlaps_device": _sig(_vp, MASK, _vp, OVERLAPS, _vp),
    "cvh_overlaps_device_batch": _sig(MEMBERS, MASK, _vpp, _vpp, _lp, _lp, _ip, _vp),
    "cvh_match_overlaps": _sig(_vp, _long, _u32, _u32, _vp, _int, C.POINTER(Match)),
    "cvh_contours": _sig(_vp, MASK, _int, LOOPS),
    "cvh_contours_device": _sig(_vp, MASK, _int, LOOPS, _vp),
    "cvh_contours_device_batch": _sig(MEMBERS, MASK, _int, LOOPS_BATCH, _vp),
    "cvh_contours_subpixel": _sig(_vp, MASK, LOOPS),
    "cvh_contours_subpixel_device": _sig(_vp, MASK, LOOPS, _vp),
    "cvh_contours_subpixel_device_batch": _sig(MEMBERS, MASK, LOOPS_BATCH, _vp),
    "cvh_contour_subpixel_measure": _sig(_vp, _long, _dp, _dp),
    "cvh_get_mask_morph": _sig(_vp, _u8p, MASK, _int, _u32),
    "cvh_get_mask_morph_device": _sig(_vp, _vp, MASK, _int, _u32, _vp),
    "cvh_get_mask_morph_device_batch": _sig(MEMBERS, _vpp, MASK, _int, _u32p, _vp),
    "cvh_morph_levelset": _sig(_vp, MASK, _int, _u32, FILL),
    "cvh_morph_levelset_batch": _sig(MEMBERS, MASK, _int, _u32p, FILL),
    "cvh_init_mask": _sig(_vp, _u8p, FILL),
    "cvh_init_mask_device": _sig(_vp, _vp, FILL, _vp),
    "cvh_init_mask_device_batch": _sig(MEMBERS, _vpp, FILL, _vp),
    "cvh_split": _sig(_vp, MASK, _u32, _vp, TABLE, _vp),
    "cvh_split_host": _sig(_vp, MASK, _u32, _vp, TABLE),
    "cvh_split_batch": _sig(MEMBERS, MASK, _u32p, _vpp, _ip, _vp),
    "cvh_split_levelset": _sig(_vp, MASK, _u32, FILL),
    "cvh_split_levelset_batch": _sig(MEMBERS, MASK, _u32p, FILL),
    "cvh_split_geometry": _sig(_ip, _ip, _ip, res=None),
    "cvh_multiphase_run": _sig(_vp, _vp, RUN, _dp, TRACE),
    "cvh_multiphase_run_batch": _sig(_vp, MARCH_MEMBERS, RUN, _vp, TRACE),
    "cvh_multiphase_means": _sig(_vp, _vp, _dp),
    "cvh_multiphase_labels": _sig(_vp, _vp, _u8p),
    "cvh_multiphase_labels_device": _sig(_vp, _vp, _vp, _vp),
    "cvh_multiphase_geometry": _sig(_int, _int, _ip, _ip, _ip, res=None),
    "cvh_localized_run": _sig(_vp, _int, RUN, _dp, TRACE),
    "cvh_localized_run_batch": _sig(MARCH_MEMBERS, _ip, RUN, _vp, TRACE),
    "cvh_localized_means": _sig(_vp, _int, _dp, _dp, _vp, _vp, _vp),
    "cvh_localized_geometry": _sig(_int, _int, _int, _ip, _ip, _ip, _ip, res=None),
    "cvh_set_edge_map": _sig(_vp, _vp),
    "cvh_get_edge_map": _sig(_vp, _vp),
    "cvh_set_edge_map_device": _sig(_vp, _vp, _vp),
    "cvh_get_edge_map_device": _sig(_vp, _vp, _vp),
    "cvh_edge_map": _sig(_vp, _vp, _dbl),
    "cvh_edge_map_batch": _sig(_vp, MARCH_MEMBERS, _dp),
    "cvh_geodesic_run": _sig(_vp, RUN, _dp, TRACE),
    "cvh_geodesic_run_batch": _sig(MARCH_MEMBERS, RUN, _vp, TRACE),
    "cvh_geodesic_geometry": _sig(_int, _int, _ip, _ip, _ip, res=None),
    "cvh_convex_run": _sig(_vp, _int, C.POINTER(ConvexParams), _ip, _dp, _dp, TRACE),
    "cvh_convex_run_batch": _sig(MARCH_MEMBERS, _int, C.POINTER(ConvexParams), _ip, _dp, _vp, TRACE),
    "cvh_get_relaxed": _sig(_vp, _dp, _dp, _dp),
    "cvh_get_relaxed_device": _sig(_vp, _vp, _vp),
    "cvh_convex_geometry": _sig(_int, _int, _ip, _ip, _ip, res=None),
}
EXPORTS = list(SIGNATURES)

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
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L
