"""The calls that start from a context's mask, raw or cleaned -- cvh_components*, cvh_get_mask_clean*, cvh_measure*, cvh_overlaps*,
cvh_contours*, cvh_get_mask_morph* / cvh_morph_levelset* / cvh_init_mask* -- and cvh_score_mask* and cvh_reinit*: the FULL text of every
refusal, which refusal wins when two faults meet, and one positive call per family.

The expected texts are written out here; none is produced by the library (a pointer's text is formatted here from its address).  A
refusal's text is what cvh_last_error(NULL) holds and what the call's member 0 holds; where a single-context form records it through the
context alone (cvh_get_mask_clean's "mask is NULL" and "no level set"), member 0 holds it and cvh_last_error(NULL) keeps what it held.
The return code is the stated one, no launch set is counted, and every context is as it was: the mask, the level set, the step count
cvh_sync reports; the context without a level set still has none and the one without an image still refuses cvh_run for that.

Contexts are 16 x 25 with one and three channels: three hold an image and a level set STEPS iterations old, one an image and no level
set, one a level set and no image.  NOT covered: the "is too large" refusals (they need planes of 2^30 pixels or more) and "is on
device %d" (needs a second GPU).  Run with -m gpu on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_device_io as DIO

pytestmark = pytest.mark.gpu
OK, ERR_ARG, ERR_STATE = 0, 1, 3
NO_IMAGE = "no image set (call cvh_set_image first)"
STEPS = 3
H, W = 16, 25
# name: (channels, holds an image, holds a level set)
CONTEXTS = {"A1": (1, True, True), "A3": (3, True, True), "C1": (1, True, True), "E1": (1, True, False), "U1": (1, False, True)}
COUNTERS = ("cvh_debug_reinit_launch_sets", "cvh_debug_score_launch_sets", "cvh_debug_morph_launch_sets", "cvh_debug_overlap_launch_sets")


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def image_of(name):
    return DIO.planes_of(DIO.rand_image(H, W, CONTEXTS[name][0], seed=sum(map(ord, name))))


@pytest.fixture(scope="module")
def K(capi):
    """the contexts of CONTEXTS, by name, and under "was" what each held before any call of this file"""
    ctxs = {name: capi.Context(H, W, ch, capi.make_params(tol=0.0)) for name, (ch, _, _) in CONTEXTS.items()}
    was = {}
    for name, c in ctxs.items():
        _, image, levelset = CONTEXTS[name]
        if image:
            c.set_image(image_of(name))
        if levelset:
            c.init_checkerboard()
        if image and levelset:
            c.enqueue_steps(STEPS)
            assert c.sync()[0] == STEPS
        if levelset:
            was[name] = (c.get_mask(), c.get_levelset())
    ctxs["was"] = was
    yield ctxs
    for name in CONTEXTS:
        ctxs[name].close()


@pytest.fixture(scope="module")
def P(capi):
    """what the calls point at: g0 .. g2, device planes of h * w int32 (zero); odd0 .. odd2, two bytes into them; host tables and planes"""
    hip = DIO.Hip()
    p = {}
    for i in range(3):
        p[f"g{i}"] = hip.upload(np.zeros((H, W), np.int32))
        p[f"odd{i}"] = p[f"g{i}"] + 2
    p["comp"] = np.zeros(8, capi.COMPONENT_DTYPE)
    p["region"] = np.zeros(8, capi.REGION_DTYPE)
    p["pairs"] = np.zeros(8, capi.OVERLAP_DTYPE)
    p["loops"] = np.zeros(8, capi.CONTOUR_LOOP_DTYPE)
    p["bytes"] = np.zeros((H, W), np.uint8)
    p["plane"] = np.zeros((H, W), np.int32)
    p["score"] = (capi.MaskScore * 3)()
    yield p
    hip.free_all()


def members(K, names):
    """a ctypes list of handles; a name of None is a NULL entry"""
    return (C.c_void_p * max(len(names), 1))(*[K[n]._h.value if n else None for n in names])


def ptrs(*v):
    return (C.c_void_p * max(len(v), 1))(*v)


def ints(*v):
    return (C.c_int * max(len(v), 1))(*v)


def longs(*v):
    return (C.c_long * max(len(v), 1))(*v)


def u32s(*v):
    return (C.c_uint32 * max(len(v), 1))(*v)


def u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def at(a):
    return a.ctypes.data


def h(K, name):
    return K[name]._h


RAW, CLEANED = (0, 0, 0), (3, 0, 0)   # min_area, fill_holes, keep_largest


def components_batch(names, labels, conn=4):
    return lambda L, K, P: L.cvh_components_batch(members(K, names), len(names), conn, 0, labels(P) if labels else None, None, None)


def clean_batch(names, masks, conn=4, opts=CLEANED):
    return lambda L, K, P: L.cvh_get_mask_clean_device_batch(members(K, names), len(names), masks(P) if masks else None, conn, 0, *opts, None)


def measure_batch(names, tables=None, caps=None, conn=4, opts=RAW):
    return lambda L, K, P: L.cvh_measure_batch(members(K, names), len(names), conn, 0, *opts, tables(P) if tables else None, caps, None, None)


def overlaps_batch(names, others, tables=None, caps=None, conn=4, opts=RAW):
    return lambda L, K, P: L.cvh_overlaps_device_batch(members(K, names), len(names), conn, 0, *opts, others(P) if others else None,
                                                       tables(P) if tables else None, caps, None, None, None)


def contours_batch(names, loops=None, loop_caps=None, points=None, point_caps=None, conn=8, opts=RAW, simplify=1):
    return lambda L, K, P: L.cvh_contours_device_batch(members(K, names), len(names), conn, 0, *opts, simplify, loops(P) if loops else None,
                                                       loop_caps, points(P) if points else None, point_caps, None, None, None)


def morph_batch(names, masks, r2=(4, 4, 4), conn=4, opts=RAW, op=1):
    return lambda L, K, P: L.cvh_get_mask_morph_device_batch(members(K, names), len(names), masks(P) if masks else None, conn, 0, *opts, op,
                                                             u32s(*r2) if r2 else None, None)


def morph_levelset_batch(names, r2=(4, 4, 4), conn=4, opts=RAW, op=1):
    return lambda L, K, P: L.cvh_morph_levelset_batch(members(K, names), len(names), conn, 0, *opts, op, u32s(*r2) if r2 else None, 1.0, -1.0)


def score_batch(names, truths, out=True):
    return lambda L, K, P: L.cvh_score_mask_device_batch(members(K, names), len(names), truths(P) if truths else None, 0, 4,
                                                         P["score"] if out else None, None)


def reinit_batch(names):
    return lambda L, K, P: L.cvh_reinit_batch(members(K, names), len(names), None)


NO_LS = "member %d has no level set"
NULL_PTR = "member %d: the device pointer is NULL"
NULL_LIST = "the list of device pointers is NULL"
ODD = "member %d: {odd%d:#x} is not aligned to 4 bytes"
# (id, call, return code, text -- its {fields} are the addresses of P --, the context that holds the text too or None, and "ctx" where
# that context alone holds it)
REFUSALS = [
    # ---- the member list: every family goes through the same check ----
    ("components-empty", lambda L, K, P: L.cvh_components_batch(None, 0, 4, 0, None, None, None), ERR_ARG,
     "cvh_components_batch: empty member list (ctxs = (nil), n = 0)", None),
    ("clean-null-member", clean_batch(["A1", None], lambda P: ptrs(P["g0"], P["g1"])), ERR_ARG,
     "cvh_get_mask_clean_device_batch: member 1 is NULL", "A1"),
    ("measure-twice", measure_batch(["A1", "A3", "A1"]), ERR_ARG, "cvh_measure_batch: member 2 duplicates member 0", "A1"),
    ("overlap-null-member-before-conn", overlaps_batch([None, "A1"], None, conn=5), ERR_ARG, "cvh_overlaps_device_batch: member 0 is NULL", None),
    ("contour-empty", lambda L, K, P: L.cvh_contours_device_batch(None, 2, 8, 0, 0, 0, 0, 1, *([None] * 7)), ERR_ARG,
     "cvh_contours_device_batch: empty member list (ctxs = (nil), n = 2)", None),
    ("morph-null-member", morph_levelset_batch(["A1", "A3", None]), ERR_ARG, "cvh_morph_levelset_batch: member 2 is NULL", "A1"),
    ("score-twice", score_batch(["A3", "A3"], lambda P: ptrs(P["g0"], P["g1"])), ERR_ARG,
     "cvh_score_mask_device_batch: member 1 duplicates member 0", "A3"),
    ("reinit-null-member", reinit_batch(["A1", None]), ERR_ARG, "cvh_reinit_batch: member 1 is NULL", "A1"),
    # ---- components ----
    ("components-conn-before-unaligned", components_batch(["A1", "A3"], lambda P: ptrs(P["odd0"], P["g1"]), conn=5), ERR_ARG,
     "cvh_components_batch: conn must be 4 or 8, got 5", "A1"),
    ("components-cap-before-unaligned", lambda L, K, P: L.cvh_components(h(K, "A1"), 4, 0, P["odd0"], at(P["comp"]), -1, None, None), ERR_ARG,
     "cvh_components: cap must not be negative, got -1", "A1"),
    ("components-conn-before-cap", lambda L, K, P: L.cvh_components(h(K, "A1"), 0, 0, None, at(P["comp"]), -1, None, None), ERR_ARG,
     "cvh_components: conn must be 4 or 8, got 0", "A1"),
    ("components-unaligned-before-no-levelset", components_batch(["E1", "A1", "A3"], lambda P: ptrs(None, P["g1"], P["odd2"])), ERR_ARG,
     "cvh_components_batch: " + ODD % (2, 2), "E1"),
    ("components-host-pointer", lambda L, K, P: L.cvh_components(h(K, "A1"), 4, 0, at(P["plane"]), None, 0, None, None), ERR_ARG,
     "cvh_components: member 0: {host_plane:#x} is not device-accessible memory of device 0", "A1"),
    ("components-no-levelset", components_batch(["A1", "A3", "E1"], None), ERR_STATE, "cvh_components_batch: " + NO_LS % 2, "A1"),
    ("components-no-levelset-single", lambda L, K, P: L.cvh_components(h(K, "E1"), 8, 0, None, None, 0, None, None), ERR_STATE,
     "cvh_components: " + NO_LS % 0, "E1"),
    # ---- the cleaned mask ----
    ("clean-conn-before-null-pointer", lambda L, K, P: L.cvh_get_mask_clean_device(h(K, "A1"), None, 6, 0, 3, 0, 0, None), ERR_ARG,
     "cvh_get_mask_clean_device: conn must be 4 or 8, got 6", "A1"),
    ("clean-min-area-before-fill-holes", clean_batch(["A1"], lambda P: ptrs(P["g0"]), opts=(-1, -2, 2)), ERR_ARG,
     "cvh_get_mask_clean_device_batch: min_area must not be negative, got -1", "A1"),
    ("clean-fill-holes-before-keep-largest", clean_batch(["A1"], lambda P: ptrs(P["g0"]), opts=(0, -2, 2)), ERR_ARG,
     "cvh_get_mask_clean_device_batch: fill_holes must be -1 (any size) or an area >= 0, got -2", "A1"),
    ("clean-keep-largest-before-null-list", clean_batch(["A1"], None, opts=(0, -1, 2)), ERR_ARG,
     "cvh_get_mask_clean_device_batch: keep_largest must be 0 or 1, got 2", "A1"),
    ("clean-null-list", clean_batch(["A1", "E1"], None), ERR_ARG, "cvh_get_mask_clean_device_batch: " + NULL_LIST, "A1"),
    ("clean-null-list-raw", clean_batch(["A1", "E1"], None, opts=RAW), ERR_ARG, "cvh_get_mask_clean_device_batch: " + NULL_LIST, "A1"),
    ("clean-null-pointer-before-no-levelset", clean_batch(["A1", "E1", "A3"], lambda P: ptrs(P["g0"], P["g1"], None)), ERR_ARG,
     "cvh_get_mask_clean_device_batch: " + NULL_PTR % 2, "A1"),
    ("clean-null-pointer-before-no-levelset-raw", clean_batch(["A1", "E1", "A3"], lambda P: ptrs(P["g0"], P["g1"], None), opts=RAW), ERR_ARG,
     "cvh_get_mask_clean_device_batch: " + NULL_PTR % 2, "A1"),
    ("clean-no-levelset", clean_batch(["A1", "A3", "E1"], lambda P: ptrs(P["g0"], P["g1"], P["g2"])), ERR_STATE,
     "cvh_get_mask_clean_device_batch: " + NO_LS % 2, "A1"),
    ("clean-no-levelset-raw", clean_batch(["A1", "A3", "E1"], lambda P: ptrs(P["g0"], P["g1"], P["g2"]), opts=RAW), ERR_STATE,
     "cvh_get_mask_clean_device_batch: " + NO_LS % 2, "A1"),
    ("clean-no-levelset-single-device", lambda L, K, P: L.cvh_get_mask_clean_device(h(K, "E1"), P["g0"], 4, 0, 0, -1, 0, None), ERR_STATE,
     "cvh_get_mask_clean_device: " + NO_LS % 0, "E1"),
    # the host form says two of its refusals in its own words, through the context alone
    ("clean-host-null-mask-before-conn", lambda L, K, P: L.cvh_get_mask_clean(h(K, "A1"), None, 5, 0, 3, 0, 0), ERR_ARG,
     "cvh_get_mask_clean: mask is NULL", "A1", "ctx"),
    ("clean-host-conn-before-no-levelset", lambda L, K, P: L.cvh_get_mask_clean(h(K, "E1"), u8(P["bytes"]), 5, 0, 3, 0, 0), ERR_ARG,
     "cvh_get_mask_clean: conn must be 4 or 8, got 5", "E1"),
    ("clean-host-no-levelset", lambda L, K, P: L.cvh_get_mask_clean(h(K, "E1"), u8(P["bytes"]), 4, 0, 3, 0, 0), ERR_STATE,
     "cvh_get_mask_clean: no level set", "E1", "ctx"),
    ("clean-host-no-levelset-raw", lambda L, K, P: L.cvh_get_mask_clean(h(K, "E1"), u8(P["bytes"]), 4, 0, 0, 0, 0), ERR_STATE,
     "cvh_get_mask_clean: no level set", "E1", "ctx"),
    # ---- measures ----
    ("measure-single-cap-before-conn", lambda L, K, P: L.cvh_measure(h(K, "A1"), 5, 0, 0, 0, 0, at(P["region"]), -1, None, None), ERR_ARG,
     "cvh_measure: cap must not be negative, got -1", "A1"),
    ("measure-conn-before-cap", measure_batch(["A1", "A3"], lambda P: ptrs(at(P["region"]), at(P["region"])), ints(-1, 1), conn=7), ERR_ARG,
     "cvh_measure_batch: conn must be 4 or 8, got 7", "A1"),
    ("measure-cap-of-member-with-table", measure_batch(["A1", "A3", "C1"], lambda P: ptrs(None, at(P["region"]), at(P["region"])), ints(-5, 2, -2)),
     ERR_ARG, "cvh_measure_batch: member 2: cap must not be negative, got -2", "A1"),
    ("measure-tables-without-caps-before-no-image", measure_batch(["A1", "U1"], lambda P: ptrs(None, at(P["region"]))), ERR_ARG,
     "cvh_measure_batch: tables without caps", "A1"),
    ("measure-min-area-before-tables-without-caps", measure_batch(["A1"], lambda P: ptrs(at(P["region"])), opts=(-4, 0, 0)), ERR_ARG,
     "cvh_measure_batch: min_area must not be negative, got -4", "A1"),
    ("measure-no-image-before-no-levelset", measure_batch(["A1", "E1", "U1"]), ERR_STATE,
     "cvh_measure_batch: member 2 has no image (call cvh_set_image first)", "A1"),
    ("measure-no-image-single", lambda L, K, P: L.cvh_measure(h(K, "U1"), 4, 0, 3, 0, 0, None, 0, None, None), ERR_STATE,
     "cvh_measure: member 0 has no image (call cvh_set_image first)", "U1"),
    ("measure-no-levelset", measure_batch(["A1", "A3", "E1"], opts=CLEANED), ERR_STATE, "cvh_measure_batch: " + NO_LS % 2, "A1"),
    ("measure-no-levelset-raw", measure_batch(["A3", "E1"]), ERR_STATE, "cvh_measure_batch: " + NO_LS % 1, "A3"),
    # ---- overlaps ----
    ("overlap-conn-before-null-list", overlaps_batch(["A1", "A3"], None, conn=6), ERR_ARG, "cvh_overlaps_device_batch: conn must be 4 or 8, got 6", "A1"),
    ("overlap-null-list-before-tables-without-caps", overlaps_batch(["A1"], None, lambda P: ptrs(at(P["pairs"]))), ERR_ARG,
     "cvh_overlaps_device_batch: " + NULL_LIST, "A1"),
    ("overlap-tables-without-caps-before-unaligned", overlaps_batch(["A1", "A3"], lambda P: ptrs(P["odd0"], P["g1"]), lambda P: ptrs(None, at(P["pairs"]))),
     ERR_ARG, "cvh_overlaps_device_batch: tables without caps", "A1"),
    ("overlap-cap-before-unaligned", lambda L, K, P: L.cvh_overlaps_device(h(K, "A1"), 4, 0, 0, 0, 0, P["odd0"], at(P["pairs"]), -1, None, None, None),
     ERR_ARG, "cvh_overlaps_device: member 0: cap must not be negative, got -1", "A1"),
    ("overlap-cap-before-null-pointer", overlaps_batch(["A1", "A3", "C1"], lambda P: ptrs(None, P["g1"], P["g2"]),
                                                       lambda P: ptrs(None, None, at(P["pairs"])), longs(-1, -1, -7)), ERR_ARG,
     "cvh_overlaps_device_batch: member 2: cap must not be negative, got -7", "A1"),
    ("overlap-null-pointer-before-no-levelset", overlaps_batch(["E1", "A1"], lambda P: ptrs(P["g0"], None)), ERR_ARG,
     "cvh_overlaps_device_batch: " + NULL_PTR % 1, "E1"),
    ("overlap-unaligned-before-no-levelset", overlaps_batch(["A1", "E1", "A3"], lambda P: ptrs(P["g0"], P["g1"], P["odd2"]), opts=CLEANED), ERR_ARG,
     "cvh_overlaps_device_batch: " + ODD % (2, 2), "A1"),
    ("overlap-host-pointer-before-unaligned", overlaps_batch(["A1", "A3"], lambda P: ptrs(at(P["plane"]), P["odd1"])), ERR_ARG,
     "cvh_overlaps_device_batch: member 0: {host_plane:#x} is not device-accessible memory of device 0", "A1"),
    ("overlap-no-levelset", overlaps_batch(["A1", "A3", "E1"], lambda P: ptrs(P["g0"], P["g1"], P["g2"])), ERR_STATE,
     "cvh_overlaps_device_batch: " + NO_LS % 2, "A1"),
    # the host form: its own NULL text, "member 0:" in front of the cap (cvh_measure has none), the level set before the plane is staged
    ("overlap-host-conn-before-null-plane", lambda L, K, P: L.cvh_overlaps(h(K, "A1"), 5, 0, 0, 0, 0, None, None, 0, None, None), ERR_ARG,
     "cvh_overlaps: conn must be 4 or 8, got 5", "A1"),
    ("overlap-host-null-plane-before-cap", lambda L, K, P: L.cvh_overlaps(h(K, "A1"), 4, 0, 0, 0, 0, None, at(P["pairs"]), -1, None, None), ERR_ARG,
     "cvh_overlaps: other is NULL", "A1"),
    ("overlap-host-cap-before-no-levelset", lambda L, K, P: L.cvh_overlaps(h(K, "E1"), 4, 0, 0, 0, 0, at(P["plane"]), at(P["pairs"]), -1, None, None),
     ERR_ARG, "cvh_overlaps: member 0: cap must not be negative, got -1", "E1"),
    ("overlap-host-no-levelset", lambda L, K, P: L.cvh_overlaps(h(K, "E1"), 4, 0, 0, 0, 0, at(P["plane"]), None, 0, None, None), ERR_STATE,
     "cvh_overlaps: " + NO_LS % 0, "E1"),
    # ---- contours ----
    ("contour-single-loop-cap-before-conn", lambda L, K, P: L.cvh_contours_device(h(K, "A1"), 5, 0, 0, 0, 0, 1, None, -1, None, -1, None, None, None),
     ERR_ARG, "cvh_contours_device: loop_cap must not be negative, got -1", "A1"),
    ("contour-single-point-cap-before-simplify", lambda L, K, P: L.cvh_contours(h(K, "A1"), 8, 0, 0, 0, 0, 2, None, 0, None, -3, None, None), ERR_ARG,
     "cvh_contours: point_cap must not be negative, got -3", "A1"),
    ("contour-conn-before-simplify", contours_batch(["A1", "A3"], conn=0, simplify=2), ERR_ARG, "cvh_contours_device_batch: conn must be 4 or 8, got 0", "A1"),
    ("contour-simplify-before-tables-without-caps", contours_batch(["A1"], lambda P: ptrs(at(P["loops"])), simplify=2), ERR_ARG,
     "cvh_contours_device_batch: simplify must be 0 or 1, got 2", "A1"),
    ("contour-loop-tables-without-caps-before-unaligned", contours_batch(["A1", "A3"], lambda P: ptrs(None, at(P["loops"])), None,
                                                                         lambda P: ptrs(P["odd0"], P["g1"]), longs(4, 4)), ERR_ARG,
     "cvh_contours_device_batch: loop tables without loop_caps", "A1"),
    ("contour-point-arrays-without-caps", contours_batch(["A1", "A3"], lambda P: ptrs(at(P["loops"]), None), longs(2, -1),
                                                         lambda P: ptrs(None, P["odd1"])), ERR_ARG,
     "cvh_contours_device_batch: point arrays without point_caps", "A1"),
    ("contour-point-cap-before-unaligned", contours_batch(["A1", "A3"], None, None, lambda P: ptrs(P["odd0"], P["g1"]), longs(4, -1)), ERR_ARG,
     "cvh_contours_device_batch: member 1: point_cap must not be negative, got -1", "A1"),
    ("contour-point-cap-of-member-0-before-loop-cap-of-member-1", contours_batch(["A1", "A3"], lambda P: ptrs(None, at(P["loops"])), longs(0, -1),
                                                                                 lambda P: ptrs(P["g0"], None), longs(-2, 0)), ERR_ARG,
     "cvh_contours_device_batch: member 0: point_cap must not be negative, got -2", "A1"),
    ("contour-loop-cap-in-member-2", contours_batch(["A1", "A3", "C1"], lambda P: ptrs(None, None, at(P["loops"])), longs(-1, -1, -9)), ERR_ARG,
     "cvh_contours_device_batch: member 2: loop_cap must not be negative, got -9", "A1"),
    ("contour-unaligned-before-no-levelset", contours_batch(["A1", "E1", "A3"], None, None, lambda P: ptrs(P["g0"], None, P["odd2"]), longs(4, 4, 4)),
     ERR_ARG, "cvh_contours_device_batch: " + ODD % (2, 2), "A1"),
    ("contour-host-pointer-in-device-form", lambda L, K, P: L.cvh_contours_device(h(K, "E1"), 8, 0, 0, 0, 0, 1, None, 0, at(P["plane"]), 4, None, None, None),
     ERR_ARG, "cvh_contours_device: member 0: {host_plane:#x} is not device-accessible memory of device 0", "E1"),
    ("contour-no-levelset-raw", contours_batch(["A1", "A3", "E1"]), ERR_STATE, "cvh_contours_device_batch: " + NO_LS % 2, "A1"),
    ("contour-no-levelset-cleaned", contours_batch(["A1", "A3", "E1"], opts=CLEANED), ERR_STATE, "cvh_contours_device_batch: " + NO_LS % 2, "A1"),
    ("contour-no-levelset-host", lambda L, K, P: L.cvh_contours(h(K, "E1"), 8, 0, 0, 0, 0, 1, None, 0, at(P["plane"]), 4, None, None), ERR_STATE,
     "cvh_contours: " + NO_LS % 0, "E1"),
    # ---- morphology and the mask starts ----
    ("morph-conn-before-op", morph_batch(["A1"], lambda P: ptrs(P["g0"]), conn=3, op=9), ERR_ARG,
     "cvh_get_mask_morph_device_batch: conn must be 4 or 8, got 3", "A1"),
    ("morph-op-before-null-radii", morph_batch(["A1", "A3"], None, r2=None, op=5), ERR_ARG,
     "cvh_get_mask_morph_device_batch: op must be CVH_MORPH_NONE (0) .. CVH_MORPH_CLOSE (4), got 5", "A1"),
    ("morph-op-negative", morph_levelset_batch(["A1"], op=-1), ERR_ARG,
     "cvh_morph_levelset_batch: op must be CVH_MORPH_NONE (0) .. CVH_MORPH_CLOSE (4), got -1", "A1"),
    ("morph-null-radii-before-null-list", morph_batch(["A1", "E1"], None, r2=None), ERR_ARG,
     "cvh_get_mask_morph_device_batch: the list of squared radii is NULL", "A1"),
    ("morph-levelset-null-radii-before-no-levelset", morph_levelset_batch(["E1", "A1"], r2=None), ERR_ARG,
     "cvh_morph_levelset_batch: the list of squared radii is NULL", "E1"),
    ("morph-null-list-before-no-levelset", morph_batch(["E1"], None), ERR_ARG, "cvh_get_mask_morph_device_batch: " + NULL_LIST, "E1"),
    ("morph-null-pointer-before-no-levelset", morph_batch(["A1", "E1", "A3"], lambda P: ptrs(P["g0"], P["g1"], None), opts=CLEANED), ERR_ARG,
     "cvh_get_mask_morph_device_batch: " + NULL_PTR % 2, "A1"),
    ("morph-no-levelset-raw", morph_batch(["A1", "A3", "E1"], lambda P: ptrs(P["g0"], P["g1"], P["g2"])), ERR_STATE,
     "cvh_get_mask_morph_device_batch: " + NO_LS % 2, "A1"),
    ("morph-no-levelset-cleaned", morph_batch(["A1", "A3", "E1"], lambda P: ptrs(P["g0"], P["g1"], P["g2"]), opts=CLEANED), ERR_STATE,
     "cvh_get_mask_morph_device_batch: " + NO_LS % 2, "A1"),
    ("morph-levelset-no-levelset-single", lambda L, K, P: L.cvh_morph_levelset(h(K, "E1"), 4, 0, 0, 0, 1, 2, 4, 1.0, -1.0), ERR_STATE,
     "cvh_morph_levelset: " + NO_LS % 0, "E1"),
    ("morph-host-null-mask-before-conn", lambda L, K, P: L.cvh_get_mask_morph(h(K, "A1"), None, 5, 0, 0, 0, 0, 1, 4), ERR_ARG,
     "cvh_get_mask_morph: mask is NULL", "A1"),
    ("morph-host-conn-before-no-levelset", lambda L, K, P: L.cvh_get_mask_morph(h(K, "E1"), u8(P["bytes"]), 5, 0, 0, 0, 0, 1, 4), ERR_ARG,
     "cvh_get_mask_morph: conn must be 4 or 8, got 5", "E1"),
    ("init-mask-host-null-mask", lambda L, K, P: L.cvh_init_mask(h(K, "A1"), None, 1.0, -1.0), ERR_ARG, "cvh_init_mask: mask is NULL", "A1"),
    ("init-mask-null-list", lambda L, K, P: L.cvh_init_mask_device_batch(members(K, ["A1", "A3"]), 2, None, 1.0, -1.0, None), ERR_ARG,
     "cvh_init_mask_device_batch: " + NULL_LIST, "A1"),
    ("init-mask-null-pointer", lambda L, K, P: L.cvh_init_mask_device_batch(members(K, ["A1", "A3", "C1"]), 3, ptrs(P["g0"], P["g1"], None), 1.0, -1.0, None),
     ERR_ARG, "cvh_init_mask_device_batch: " + NULL_PTR % 2, "A1"),
    # ---- scores ----
    ("score-out-before-null-list", score_batch(["A1", "A3"], None, out=False), ERR_ARG, "cvh_score_mask_device_batch: out is NULL", "A1"),
    ("score-null-list-before-no-levelset", score_batch(["E1"], None), ERR_ARG, "cvh_score_mask_device_batch: " + NULL_LIST, "E1"),
    ("score-null-pointer-before-no-levelset", score_batch(["A1", "E1", "A3"], lambda P: ptrs(P["g0"], P["g1"], None)), ERR_ARG,
     "cvh_score_mask_device_batch: " + NULL_PTR % 2, "A1"),
    ("score-no-levelset", score_batch(["A1", "A3", "E1"], lambda P: ptrs(P["g0"], P["g1"], P["g2"])), ERR_STATE,
     "cvh_score_mask_device_batch: " + NO_LS % 2, "A1"),
    ("score-host-null-truth-before-null-out", lambda L, K, P: L.cvh_score_mask(h(K, "A1"), None, 0, 4, None), ERR_ARG,
     "cvh_score_mask: truth is NULL", "A1"),
    ("score-host-null-out-before-no-levelset", lambda L, K, P: L.cvh_score_mask(h(K, "E1"), u8(P["bytes"]), 0, 4, None), ERR_ARG,
     "cvh_score_mask: out is NULL", "E1"),
    ("score-host-no-levelset", lambda L, K, P: L.cvh_score_mask(h(K, "E1"), u8(P["bytes"]), 0, 4, P["score"]), ERR_STATE,
     "cvh_score_mask: " + NO_LS % 0, "E1"),
    # ---- reinitialisation ----
    ("reinit-no-levelset", reinit_batch(["A1", "A3", "E1"]), ERR_STATE, "cvh_reinit_batch: " + NO_LS % 2, "A1"),
    ("reinit-no-levelset-single", lambda L, K, P: L.cvh_reinit(h(K, "E1"), None), ERR_STATE, "cvh_reinit: " + NO_LS % 0, "E1"),
    ("reinit-twice-before-no-levelset", reinit_batch(["E1", "A1", "A1"]), ERR_ARG, "cvh_reinit_batch: member 2 duplicates member 1", "E1"),
]


def counters(L):
    out = []
    for name in COUNTERS:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = C.c_ulong, []
        out.append(fn())
    return out


def assert_contexts_as_they_were(capi, K):
    for name, (_, image, levelset) in CONTEXTS.items():
        c = K[name]
        if image:
            assert all(np.array_equal(a, b) for a, b in zip(c.get_image(), image_of(name))), name
        if levelset:
            mask, u = K["was"][name]
            assert np.array_equal(c.get_mask(), mask), name
            assert np.array_equal(c.get_levelset(), u), name
        if image and levelset:
            assert c.sync()[0] == STEPS, name
        elif levelset:
            with pytest.raises(capi.CvhError) as e:
                c.run(1)
            assert e.value.code == ERR_STATE and str(e.value).endswith(NO_IMAGE), name
        else:
            assert capi.lib().cvh_get_mask(c._h, u8(np.zeros((H, W), np.uint8)), 0) == ERR_STATE, name


@pytest.mark.parametrize("case", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_text_code_and_untouched_contexts(capi, K, P, case):
    _, call, code, text, holder = case[:5]
    L = capi.lib()
    text = text.format(host_plane=at(P["plane"]), **{k: v for k, v in P.items() if isinstance(v, int)})
    before, launched = L.cvh_last_error(None).decode(), counters(L)
    rc = call(L, K, P)
    got = L.cvh_last_error(None).decode()
    print(rc, repr(got), repr(L.cvh_last_error(K[holder]._h).decode()) if holder else None)
    if len(case) > 5:   # recorded through the context alone
        assert got == before
    else:
        assert got == text
    assert rc == code
    if holder:
        assert L.cvh_last_error(K[holder]._h).decode() == text
    assert counters(L) == launched
    assert_contexts_as_they_were(capi, K)


# ---- one positive call per family, on the same contexts: they are as they were afterwards ----

def test_one_call_per_family_leaves_the_contexts_as_they_were(capi, K, P):
    L = capi.lib()
    names = ["A1", "A3", "C1"]
    ctxs, n = members(K, names), 3
    hip = DIO.Hip()
    try:
        labels = [hip.upload(np.zeros((H, W), np.int32)) for _ in names]
        masks = [hip.upload(np.zeros((H, W), np.uint8)) for _ in names]
        points = [hip.upload(np.zeros((4 * H * W, 2), np.int32)) for _ in names]
        raw = [K["was"][name][0] for name in names]
        counts, counts2 = ints(0, 0, 0), ints(0, 0, 0)
        assert L.cvh_components_batch(ctxs, n, 4, 0, ptrs(*labels), counts, None) == OK, L.cvh_last_error(None)
        assert_contexts_as_they_were(capi, K)
        got = [hip.get(p, (H, W), np.int32) for p in labels]
        for g, m, k in zip(got, raw, counts):
            assert np.array_equal(g != 0, m != 0) and g.max() == k
        assert L.cvh_get_mask_clean_device_batch(ctxs, n, ptrs(*masks), 4, 0, 1, -1, 0, None) == OK, L.cvh_last_error(None)
        assert_contexts_as_they_were(capi, K)
        for p, m in zip(masks, raw):   # holes filled, nothing dropped: a superset of the raw mask
            filled = hip.get(p, (H, W), np.uint8)
            assert set(np.unique(filled)) <= {0, 1} and np.all(filled >= m)
        tables = [np.zeros(H * W, capi.REGION_DTYPE) for _ in names]
        assert L.cvh_measure_batch(ctxs, n, 4, 0, 0, 0, 0, ptrs(*[at(t) for t in tables]), ints(*[H * W] * 3), counts2, None) == OK, L.cvh_last_error(None)
        assert_contexts_as_they_were(capi, K)
        for t, m, k, k2 in zip(tables, raw, counts, counts2):
            assert k2 == k and int(t["area"][:k].sum()) == int(m.sum())
        rows = [np.zeros(H * W + 1, capi.OVERLAP_DTYPE) for _ in names]
        pairs = longs(0, 0, 0)
        assert L.cvh_overlaps_device_batch(ctxs, n, 4, 0, 0, 0, 0, ptrs(*labels), ptrs(*[at(r) for r in rows]), longs(*[H * W + 1] * 3), pairs, counts2,
                                           None) == OK, L.cvh_last_error(None)
        assert_contexts_as_they_were(capi, K)
        for r, m, k, k2, p in zip(rows, raw, counts, counts2, pairs):   # against its own labels: every component meets itself alone
            assert k2 == k and p == k + (1 if (m == 0).any() else 0)
            assert all(int(a) == int(b) for a, b in zip(r["a"][:p], r["b"][:p])) and int(r["count"][:p].sum()) == H * W
        nloops, npoints = longs(0, 0, 0), longs(0, 0, 0)
        assert L.cvh_contours_device_batch(ctxs, n, 4, 0, 0, 0, 0, 0, None, None, ptrs(*points), longs(*[4 * H * W] * 3), nloops, npoints,
                                           None) == OK, L.cvh_last_error(None)
        assert_contexts_as_they_were(capi, K)
        for m, k, nl, npt in zip(raw, counts, nloops, npoints):
            assert nl >= k and (npt > 0) == bool(m.any())
        assert L.cvh_get_mask_morph_device_batch(ctxs, n, ptrs(*masks), 4, 0, 0, 0, 0, 0, u32s(0, 0, 0), None) == OK, L.cvh_last_error(None)
        assert_contexts_as_they_were(capi, K)
        for p, m in zip(masks, raw):   # CVH_MORPH_NONE of the raw mask
            assert np.array_equal(hip.get(p, (H, W), np.uint8), m)
        out = (capi.MaskScore * 3)()
        assert L.cvh_score_mask_device_batch(ctxs, n, ptrs(*masks), 0, 4, out, None) == OK, L.cvh_last_error(None)
        assert_contexts_as_they_were(capi, K)
        for s, m in zip(out, raw):   # against itself
            assert (s.tp, s.fp, s.fn, s.tn) == (int(m.sum()), 0, 0, int((m == 0).sum()))
    finally:
        hip.free_all()


def test_reinit_keeps_the_mask_and_begins_a_run(capi, K):
    name = "A3"
    with capi.Context(H, W, 3, capi.make_params(tol=0.0)) as c:
        c.set_image(image_of(name))
        c.set_levelset(K["was"][name][1])
        changed = c.reinit()
        mask = K["was"][name][0]
        assert changed == bool(mask.any() and (mask == 0).any())
        assert np.array_equal(c.get_mask(), mask)
        assert c.sync()[0] == 0
    assert_contexts_as_they_were(capi, K)
