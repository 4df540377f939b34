"""What chan_vese_amd/capi.py hands to the library, call by call, without a GPU and without a built library: the loaded library is replaced
by a recording stand-in before the first lib() call (ctypes.CDLL and the path check are patched), every public wrapper and every Context
method is called once per form with fixed arguments, and every library call is printed as (name, normalised arguments) beside the wrapper's
return value.  Two trees marshal alike when their transcripts are identical:
    python tools/capi_transcript.py --full > transcript.txt
Without --full the transcript is condensed to one line per wrapper: its forms, its library calls and a digest of the full text.

Each case runs three times: "rows" (every call returns CVH_OK, count outputs are filled with small fixed numbers so that second passes
happen), "empty" (the same with counts of 0) and "error" (every call returns 7: which message the wrapper reads -- cvh_last_error of the
context's handle or of NULL -- and what it raises).  Normalisation: ctypes arrays become lists, None stays None, a numpy buffer (as a
typed pointer or as its address, also inside a pointer array) becomes [dtype, size] (+ the byte offset where a call points into it),
byref(x) becomes "&" + the type's name.  The names of the output parameters come from include/chanvese_hip.h."""
import ctypes as C
import dataclasses
import hashlib
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILL = {"count": 3, "counts": 3, "pairs": 4, "nloops": 2, "npoints": 5, "rows": 2, "bins": 3, "steps_done": 7, "steps_done_total": 7, "stopped": 1,
        "changed": 1, "t": 100}
COUNTS = ("count", "counts", "pairs", "nloops", "npoints", "rows", "bins")
DEFAULTS = {"int": 1, "long": 1, "double": 0.5, "float": 1.5}
BYREF = type(C.byref(C.c_int()))


def header_params():
    """{name: [(const, base type, levels of pointer, parameter name)]} of every declaration of the header"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chanvese_hip.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^[\w \*]+?\b(cvh_\w+)\(([^;]*?)\);", hdr, flags=re.M | re.S):
        params = []
        for p in (q.strip() for q in m.group(2).split(",")):
            if p and p != "void":
                words = re.findall(r"\w+", p)
                params.append((p.startswith("const"), [w for w in words[:-1] if w != "const"][0], p.count("*"), words[-1]))
        out[m.group(1)] = params
    return out


class Buffers:
    """the numpy arrays the binding made, by address (kept alive, so no address comes twice)"""

    def __init__(self):
        self.kept = []

    def keep(self, a):
        if isinstance(a, np.ndarray):
            self.kept.append(a)
        return a

    def find(self, address):
        for a in reversed(self.kept):
            start = a.ctypes.data
            if start <= address < start + max(a.nbytes, 1):
                return [dtype_name(a.dtype), a.size] + ([address - start] if address != start else [])
        return "address?"


def dtype_name(dtype):
    return str(dtype) if dtype.names is None else f"record of {dtype.itemsize} bytes"


BUFFERS = Buffers()


class NumpyKeeping:
    """numpy, with the array makers the binding uses reporting to BUFFERS"""

    def __getattr__(self, name):
        return getattr(np, name)

    def zeros(self, *a, **k):
        return BUFFERS.keep(np.zeros(*a, **k))

    def empty(self, *a, **k):
        return BUFFERS.keep(np.empty(*a, **k))

    def empty_like(self, *a, **k):
        return BUFFERS.keep(np.empty_like(*a, **k))

    def ascontiguousarray(self, *a, **k):
        return BUFFERS.keep(np.ascontiguousarray(*a, **k))


def norm(a):
    if a is None or isinstance(a, (bool, float, str)):
        return a
    if isinstance(a, bytes):
        return a.decode()
    if isinstance(a, int):
        return BUFFERS.find(a) if a >= 1 << 32 else a
    if isinstance(a, BYREF):
        return "&" + type(a._obj).__name__
    if isinstance(a, C.Array):
        if issubclass(a._type_, C._Pointer):
            return [BUFFERS.find(C.cast(e, C.c_void_p).value) for e in a]
        if a._type_ is C.c_char or issubclass(a._type_, C.Structure):
            return f"{a._type_.__name__}[{len(a)}]"
        return [norm(v) for v in a]
    if isinstance(a, C._Pointer):
        arr = getattr(a, "_arr", None)
        return "pointer?" if arr is None else [dtype_name(arr.dtype), arr.size]
    if isinstance(a, C._SimpleCData):
        return {type(a).__name__: norm(a.value)}
    return f"?{type(a).__name__}"


def shown(v):
    """a wrapper's return value: arrays by dtype and shape (np.empty leaves their contents open), records by their fields"""
    if isinstance(v, np.ndarray):
        return ["ndarray", dtype_name(v.dtype), list(v.shape)]
    if isinstance(v, np.generic):
        return v.item()
    if dataclasses.is_dataclass(v):
        return repr(v)
    if isinstance(v, C.Structure):
        return [type(v).__name__] + [list(x) if isinstance(x, C.Array) else x for x in (getattr(v, f[0]) for f in v._fields_)]
    if isinstance(v, (tuple, list)):
        return [shown(x) for x in v]
    if isinstance(v, dict):
        return {str(k): shown(x) for k, x in v.items()}
    return v


class Function:
    def __init__(self, lib, name):
        self.lib, self.name, self.restype, self.argtypes = lib, name, C.c_int, None

    def __call__(self, *args):
        lib = self.lib
        if self.name != "cvh_destroy" or lib.log_destroy:
            lib.log.append((self.name, [norm(a) for a in args]))
        if self.name == "cvh_last_error":
            return b"the stand-in's message"
        if self.name == "cvh_version":
            return b"stand-in"
        if self.restype is None:
            self.fill(args)
            return None
        if lib.mode == "error":
            return 7
        self.fill(args)
        return 0

    def fill(self, args):
        for (const, base, pointer, pname), a in zip(self.lib.params[self.name], args):
            if not pointer or const or a is None:
                continue
            if base == "cvh_context" and pointer == 2 and isinstance(a, BYREF):
                self.lib.handles += 0x1000
                a._obj.value = self.lib.handles
            elif base == "char" and isinstance(a, C.Array):
                a.value = b"kernel=csv_kernel<1, true> grid=4 block=256"
            elif base in DEFAULTS and pointer == 1:
                value = FILL.get(pname, DEFAULTS[base])
                if self.lib.mode == "empty" and pname in COUNTS:
                    value = 0
                if isinstance(a, BYREF):
                    a._obj.value = value
                elif isinstance(a, C.Array):
                    for i in range(len(a)):
                        a[i] = value


class Library:
    def __init__(self):
        self.params, self.log, self.mode, self.handles, self.log_destroy = header_params(), [], "rows", 0, False

    def __getattr__(self, name):
        if not name.startswith("cvh_"):
            raise AttributeError(name)
        fn = Function(self, name)
        setattr(self, name, fn)
        return fn


LIB = Library()
_exists = os.path.exists
C.CDLL = lambda path, *a, **k: LIB
os.path.exists = lambda p: True if str(p).endswith("libchanvese_hip.so") else _exists(p)

from chan_vese_amd import capi   # noqa: E402

capi.lib()
capi.np = NumpyKeeping()

H, W = 32, 48
D1, D2, D3, STREAM = 0x7100, 0x7200, 0x7300, 0x99
CASES = []


def run_cases(out, full):
    """full: every call of every case; else one line per wrapper -- its forms, its library calls and a digest of their full text"""
    groups = {}
    for label, fn in CASES:
        lines = groups.setdefault(label if full else label.rsplit(" ", 1)[0], [])
        for mode in ("rows", "empty", "error"):
            LIB.mode, LIB.log = mode, []
            try:
                result = ["returns", shown(fn())]
            except capi.CvhError as e:
                result = ["raises", "CvhError", str(e)]
            except Exception as e:   # (the texts of the argument errors are free to change)
                result = ["raises", type(e).__name__]
            lines.append(f"== {label} [{mode}]\n")
            lines += [f"   {name} {json.dumps(args)}\n" for name, args in LIB.log]
            lines.append(f"   -> {json.dumps(result)}\n")
    for key, lines in groups.items():
        if full:
            out.write("".join(lines))
        else:
            forms, calls = sum(l.startswith("==") for l in lines) // 3, sum(l.startswith("   cvh_") for l in lines)
            out.write(f"{key}: {forms} forms, {calls} calls, sha256 {hashlib.sha256(''.join(lines).encode()).hexdigest()[:16]}\n")


LIB.mode = "rows"
a, b, c = capi.Context(H, W, 1), capi.Context(H, W, 1), capi.Context(H, W, 3)
d3 = capi.Context(H, W, 3)
p0, p1 = capi.Context(64, 64, 1), capi.Context(32, 32, 1)
q0, q1 = capi.Context(64, 64, 1), capi.Context(32, 32, 1)
img = lambda: np.zeros((H, W), np.uint8)
CLEAN = dict(conn=8, invert=True, min_area=5, fill_holes=-1, keep_largest=True)


def cases(prefix, **forms):
    for k, fn in forms.items():
        CASES.append((f"{prefix} {k}", fn))


# ---- module level
cases("make_params", default=lambda: capi.make_params(), all=lambda: capi.make_params(0.1, 0.2, 0.3, 0.4, 0.5, [1, 2, 3], [4, 5]))
cases("device_count", one=lambda: capi.device_count())
cases("pm_trip_count", one=lambda: capi.pm_trip_count(0.25, 20))
cases("checkerboard_host", one=lambda: capi.checkerboard_host(8, 16))
cases("ppf_apply", default=lambda: capi.ppf_apply(np.zeros((4, 8)), capi.OP_DELTA), some=lambda: capi.ppf_apply(np.zeros((4, 8)), capi.OP_HEAVISIDE, 2.0, 3, 9, 1))
cases("Context", create=lambda: capi.Context(16, 24, 3, capi.make_params(), 1).channels)
cases("enqueue_steps_batch", two=lambda: capi.enqueue_steps_batch([a, b], 5), none=lambda: capi.enqueue_steps_batch([], 5),
      iterator=lambda: capi.enqueue_steps_batch(iter([a, c]), 2))
cases("run_batch", two=lambda: capi.run_batch([a, c]), bound=lambda: capi.run_batch((a, b, c), 9), none=lambda: capi.run_batch([]))
cases("perona_malik_batch", scalars=lambda: capi.perona_malik_batch([a, b]), per_member=lambda: capi.perona_malik_batch([a, b], [1, 2], (3.0, 4.0), np.array([5, 6])),
      mixed=lambda: capi.perona_malik_batch([a, b, c], 7, [0.1, 0.2, 0.3], 2), wrong=lambda: capi.perona_malik_batch([a, b, c], [1, 2]),
      none=lambda: capi.perona_malik_batch([]))
cases("set_image_device_batch", default=lambda: capi.set_image_device_batch([a, b], [D1, D2]),
      some=lambda: capi.set_image_device_batch([a, c], (D1, 0), capi.LAYOUT_INTERLEAVED, STREAM), wrong=lambda: capi.set_image_device_batch([a, c], [D1]))
cases("init_checkerboard_batch", two=lambda: capi.init_checkerboard_batch([a, c]), none=lambda: capi.init_checkerboard_batch([]))
cases("get_mask_device_batch", default=lambda: capi.get_mask_device_batch([a, b], [D1, D2]), some=lambda: capi.get_mask_device_batch([a], [D1], True, STREAM))
cases("reinit_batch", two=lambda: capi.reinit_batch([a, c]), none=lambda: capi.reinit_batch([]))
cases("components_batch", default=lambda: capi.components_batch([a, b]), some=lambda: capi.components_batch([a, b], [D1, 0], 8, True, STREAM),
      wrong=lambda: capi.components_batch([a, b], [D1]))
cases("get_mask_clean_device_batch", default=lambda: capi.get_mask_clean_device_batch([a, b], [D1, D2]),
      some=lambda: capi.get_mask_clean_device_batch([a, b], [D1, D2], **CLEAN, stream=STREAM))
cases("otsu_from_histogram", one=lambda: capi.otsu_from_histogram([1, 2, 3, 4]), empty=lambda: capi.otsu_from_histogram([]))
cases("histogram_batch", all=lambda: capi.histogram_batch([a, c]), caps=lambda: capi.histogram_batch([a, c], [4, 0]),
      wrong=lambda: capi.histogram_batch([a, c], [4]), none=lambda: capi.histogram_batch([]))
cases("init_threshold_batch", scalar=lambda: capi.init_threshold_batch([a, b], 100), per_member=lambda: capi.init_threshold_batch([a, b], [90, 110], 2.0, -2.0),
      wrong=lambda: capi.init_threshold_batch([a, b], [1, 2, 3]))
cases("init_otsu_batch", default=lambda: capi.init_otsu_batch([a, c]), some=lambda: capi.init_otsu_batch([a], 2.0, -3.0))
cases("init_rect_batch", one_row=lambda: capi.init_rect_batch([a, b], (1, 2, 3, 4)), rows=lambda: capi.init_rect_batch([a, b], [(1, 2, 3, 4), (5, 6, 7, 8)], 2.0, 1.0),
      wrong_rows=lambda: capi.init_rect_batch([a, b], [(1, 2, 3, 4)]), wrong_width=lambda: capi.init_rect_batch([a, b], [(1, 2, 3), (4, 5, 6)]))
cases("init_disk_batch", one_row=lambda: capi.init_disk_batch([a, b], (1, 2, 3)), rows=lambda: capi.init_disk_batch([a, b], [(1, 2, 3), (5, 6, 7)], 2.0, 1.0))
cases("pyramid_shapes", three=lambda: capi.pyramid_shapes(100, 70, 3), wrong=lambda: capi.pyramid_shapes(20, 20, 3))
cases("restrict_image_batch", pairs=lambda: capi.restrict_image_batch([p0, q0], [p1, q1]), wrong=lambda: capi.restrict_image_batch([p0, q0], [p1]),
      none=lambda: capi.restrict_image_batch([], []))
cases("prolong_levelset_batch", pairs=lambda: capi.prolong_levelset_batch([p1, q1], [p0, q0]), wrong=lambda: capi.prolong_levelset_batch([p1], []))
cases("codes", colour=lambda: [capi.colour_space_code("YUV"), capi.order_code("rgb")], local=lambda: [capi.local_what_codes("stack"), capi.local_radius(3)],
      rank=lambda: [capi.rank_what_codes("median"), capi.rank_radius(7, (3,)), capi.rank_radius(127)], morph=lambda: [capi.morph_code("open"), capi.morph_code(None)],
      squares=lambda: [capi.score_tol2(2.5), capi.r2_of(1.5)])
cases("convert_colour_batch", default=lambda: capi.convert_colour_batch([c, d3], "ycrcb"), some=lambda: capi.convert_colour_batch([c], "yuv", "rgb", True),
      wrong=lambda: capi.convert_colour_batch([c], "hsv"))
cases("luma_image_batch", default=lambda: capi.luma_image_batch([c, d3], [a, b]), some=lambda: capi.luma_image_batch([c], [a], "rgb"),
      wrong=lambda: capi.luma_image_batch([c, d3], [a]))
cases("local_planes_batch", one=lambda: capi.local_planes_batch([a, b], [c, d3], 2, "stack"),
      per_pair=lambda: capi.local_planes_batch([a, b], [c, d3], [2, 3], [(1, 2), "mean"]), wrong=lambda: capi.local_planes_batch([a, b], [c, d3], [2], "mean"))
cases("rank_planes_batch", one=lambda: capi.rank_planes_batch([a, b], [c, d3], 2, "median"),
      per_pair=lambda: capi.rank_planes_batch([a, b], [c, d3], [2, 30], [(3,), "tophat"]), wrong=lambda: capi.rank_planes_batch([a, b], [c, d3], 9, "median"))
cases("run_coarse_to_fine", default=lambda: capi.run_coarse_to_fine([p0, p1]), bound=lambda: capi.run_coarse_to_fine([p0, p1], 6))
cases("run_coarse_to_fine_batch", two=lambda: capi.run_coarse_to_fine_batch([[p0, p1], [q0, q1]], 6), wrong=lambda: capi.run_coarse_to_fine_batch([[p0, p1], [q0]]))
cases("run_with_reinit", whole=lambda: capi.run_with_reinit(a, 10), segments=lambda: capi.run_with_reinit(a, 10, 4))
cases("run_batch_with_reinit", whole=lambda: capi.run_batch_with_reinit([a, b], 10), segments=lambda: capi.run_batch_with_reinit([a, b], -1, 4))
cases("energy_batch", two=lambda: capi.energy_batch([a, c]), none=lambda: capi.energy_batch([]))
cases("score_batch", default=lambda: capi.score_batch([a, b], [D1, D2]), some=lambda: capi.score_batch([a, b], [D1, 0], True, 3.0, STREAM),
      wrong=lambda: capi.score_batch([a, b], [D1]))
cases("mask_morph_batch", r2=lambda: capi.mask_morph_batch([a, b], [D1, D2], "dilate", r2=4),
      radii=lambda: capi.mask_morph_batch([a, b], [D1, D2], capi.MORPH_OPEN, radius=[1.5, 2], **CLEAN, stream=STREAM),
      r2s=lambda: capi.mask_morph_batch([a, b], [D1, D2], "close", r2=[4, 9]), neither=lambda: capi.mask_morph_batch([a, b], [D1, D2], "none"),
      wrong=lambda: capi.mask_morph_batch([a, b], [D1, D2], "erode", radius=[1, 2, 3]), both=lambda: capi.mask_morph_batch([a], [D1], "erode", r2=1, radius=1))
cases("morph_levelset_batch", r2=lambda: capi.morph_levelset_batch([a, b], "erode", r2=2), radii=lambda: capi.morph_levelset_batch([a, b], "open", radius=(1, 2), **CLEAN,
                                                                                                                     inside=2.0, outside=0.0))
cases("split_geometry", one=lambda: capi.split_geometry())
cases("split_batch", default=lambda: capi.split_batch([a, b], radius=3), some=lambda: capi.split_batch([a, b], [D1, 0], r2=[4, 9], **CLEAN, stream=STREAM),
      wrong=lambda: capi.split_batch([a, b], r2=[4]))
cases("split_levelset_batch", default=lambda: capi.split_levelset_batch([a, b], radius=3),
      some=lambda: capi.split_levelset_batch([a, b], r2=[4, 9], **CLEAN, inside=2.0, outside=0.0))
cases("init_mask_batch", default=lambda: capi.init_mask_batch([a, b], [D1, D2]), some=lambda: capi.init_mask_batch([a], [D1], 2.0, 0.0, STREAM))
cases("measure_batch", all=lambda: capi.measure_batch([a, c]), cap=lambda: capi.measure_batch([a, c], **CLEAN, cap=2, stream=STREAM),
      caps=lambda: capi.measure_batch([a, c], cap=[5, 0]), cap0=lambda: capi.measure_batch([a, c], cap=0), wrong=lambda: capi.measure_batch([a, c], cap=[5]),
      none=lambda: capi.measure_batch([]))
cases("overlaps_batch", all=lambda: capi.overlaps_batch([a, c], [D1, D2]), cap=lambda: capi.overlaps_batch([a, c], [D1, D2], **CLEAN, cap=2, stream=STREAM),
      caps=lambda: capi.overlaps_batch([a, c], [D1, D2], cap=[5, 0]), wrong=lambda: capi.overlaps_batch([a, c], [D1, D2], cap=[5]),
      wrong_planes=lambda: capi.overlaps_batch([a, c], [D1]))
ROWS = [(0, 1, 5), (1, 1, 9), (1, 2, 1), (2, 0, 4)]
cases("match_overlaps", default=lambda: capi.match_overlaps(np.array([r + (0,) for r in ROWS], dtype=capi.OVERLAP_DTYPE)),
      number=lambda: capi.match_overlaps(np.array([r + (0,) for r in ROWS], dtype=capi.OVERLAP_DTYPE), 0.75),
      empty=lambda: capi.match_overlaps(np.zeros(0, dtype=capi.OVERLAP_DTYPE), (3, 4)))
cases("contours_batch", counts_first=lambda: capi.contours_batch([a, c]), loop_caps=lambda: capi.contours_batch([a, c], loop_caps=[4, 0]),
      points=lambda: capi.contours_batch([a, c], [D1, 0], [10, 0], **CLEAN, simplify=False, loop_caps=[1, 2], stream=STREAM),
      wrong_caps=lambda: capi.contours_batch([a, c], loop_caps=[4]), wrong_points=lambda: capi.contours_batch([a, c], [D1], [10, 0]))
cases("contours_subpixel_batch", counts_first=lambda: capi.contours_subpixel_batch([a, c]),
      points=lambda: capi.contours_subpixel_batch([a, c], [D1, D2], [10, 20], **CLEAN, loop_caps=[1, 2], stream=STREAM))
LOOPS = lambda: np.array([(0, 4, 3, 0, 0, 8), (9, 4, 0, 0, 3, -2), (5, 4, 2, 0, 3, 2)], dtype=capi.CONTOUR_LOOP_DTYPE)
cases("contour_subpixel_measures", three=lambda: capi.contour_subpixel_measures(LOOPS(), np.zeros((5, 2))),
      short=lambda: capi.contour_subpixel_measures(LOOPS(), np.zeros((4, 2))))
cases("region_shapes", two=lambda: capi.region_shapes(np.zeros(2, dtype=capi.REGION_DTYPE), 3), none=lambda: capi.region_shapes(np.zeros(0, dtype=capi.REGION_DTYPE), 1))
cases("geometry", multiphase=lambda: capi.multiphase_geometry(64, 96), localized=lambda: capi.localized_geometry(64, 96, 5), geodesic=lambda: capi.geodesic_geometry(64, 96))
TRACES = {"no_trace": dict(), "none": dict(trace=None), "bound": dict(max_steps=6), "all_rows": dict(max_steps=6, trace=True), "rows": dict(trace=4),
          "zero_rows": dict(max_steps=0, trace=True), "unbounded": dict(trace=True)}
for k, kw in TRACES.items():
    cases(f"multiphase_run {k}", one=lambda kw=kw: capi.multiphase_run(c, d3, **kw), batch=lambda kw=kw: capi.multiphase_run_batch([(a, b), (c, d3)], **kw))
    cases(f"localized_run {k}", one=lambda kw=kw: capi.localized_run(c, 5, **kw), batch=lambda kw=kw: capi.localized_run_batch([a, c], 5, **kw),
          radii=lambda kw=kw: capi.localized_run_batch([a, c], [5, 7], **kw))
    cases(f"geodesic_run {k}", one=lambda kw=kw: capi.geodesic_run(c, **kw), batch=lambda kw=kw: capi.geodesic_run_batch([a, c], **kw))
cases("march batches", no_pairs=lambda: capi.multiphase_run_batch([]), not_pairs=lambda: capi.multiphase_run_batch([(a, b, c)]),
      no_members=lambda: capi.localized_run_batch([], 5), wrong_radii=lambda: capi.localized_run_batch([a, c], [5]), no_geodesic=lambda: capi.geodesic_run_batch([]))
cases("multiphase_means", one=lambda: capi.multiphase_means(c, d3))
cases("edge_map_batch", scalar=lambda: capi.edge_map_batch([a, c], [b, d3], 4.0), per_pair=lambda: capi.edge_map_batch([a, c], [a, c], [4, 5.5]),
      wrong=lambda: capi.edge_map_batch([a, c], [a, c], [4]), unpaired=lambda: capi.edge_map_batch([a, c], [a], 4), none=lambda: capi.edge_map_batch([], [], 4))
cases("run_monitored", whole=lambda: capi.run_monitored(a, 10, 0), segments=lambda: capi.run_monitored(a, 10, 4, 0.01), wrong=lambda: capi.run_monitored(a, 10, 0, 0.01))
cases("run_batch_monitored", whole=lambda: capi.run_batch_monitored([a, c], 10, 0), segments=lambda: capi.run_batch_monitored([a, c], -1, 4))


# ---- Context
def closing():
    LIB.log_destroy = True
    try:
        with capi.Context(16, 16) as t:
            t.close()
        capi.Context(16, 16).close()
    finally:
        LIB.log_destroy = False


cases("Context.close", twice=closing)
cases("Context.set_params", one=lambda: a.set_params(capi.make_params()))
cases("Context.set_option", some=lambda: a.set_option("kernel", 3), co_resident=lambda: [p1.set_option("co_resident", 5), p1.co_resident])
cases("Context.set_image", one=lambda: a.set_image([img()]), three=lambda: c.set_image([img(), img().astype(np.int32), img()]))
for name in ("set_image_device", "get_image_device", "set_levelset_device", "get_levelset_device", "get_mask_device"):
    cases(f"Context.{name}", default=lambda name=name: getattr(c, name)(D1), some=lambda name=name: getattr(c, name)(D1, 1, STREAM),
          null=lambda name=name: getattr(c, name)(0))
cases("Context.get_image", three=lambda: c.get_image())
cases("Context.set_levelset", one=lambda: a.set_levelset(np.zeros((H, W), np.float32)))
cases("Context.init_checkerboard", one=lambda: a.init_checkerboard())
cases("Context.histogram", all=lambda: c.histogram(), cap=lambda: c.histogram(2), cap0=lambda: c.histogram(0))
cases("Context.otsu_threshold", one=lambda: a.otsu_threshold())
cases("Context.init_threshold", default=lambda: a.init_threshold(100), some=lambda: a.init_threshold(100.0, 2.0, 0.0))
cases("Context.init_otsu", default=lambda: a.init_otsu(), some=lambda: a.init_otsu(2.0, 0.0))
cases("Context.init_rect", default=lambda: a.init_rect(1, 2, 3, 4), some=lambda: a.init_rect(1, 2, 3, 4, 2.0, -1.0))
cases("Context.init_disk", default=lambda: a.init_disk(1, 2, 3), some=lambda: a.init_disk(1, 2, 3, 2.0, -1.0))
cases("Context.restrict_image_to", one=lambda: p0.restrict_image_to(p1))
cases("Context.prolong_levelset_to", one=lambda: p1.prolong_levelset_to(p0))
cases("Context.convert_colour", default=lambda: c.convert_colour("ycrcb"), some=lambda: c.convert_colour("yuv", "rgb", True), wrong=lambda: c.convert_colour("yuv", "gbr"))
cases("Context.luma_to", default=lambda: c.luma_to(a), some=lambda: c.luma_to(a, "rgb"))
cases("Context.local_planes_to", name=lambda: a.local_planes_to(c, 3, "stack"), codes=lambda: a.local_planes_to(b, 0, (2,)), wrong=lambda: a.local_planes_to(b, 128, "mean"))
cases("Context.rank_planes_to", name=lambda: a.rank_planes_to(c, 3, "median"), codes=lambda: a.rank_planes_to(b, 100, (6, 3)), wrong=lambda: a.rank_planes_to(b, 8, "median"))
cases("Context.reinit", one=lambda: a.reinit())
cases("Context.get_levelset", one=lambda: a.get_levelset())
cases("Context.run", default=lambda: a.run(), bound=lambda: a.run(12))
cases("Context.enqueue_steps", one=lambda: a.enqueue_steps(20))
cases("Context.warm", one=lambda: a.warm(20))
cases("Context.sync", one=lambda: a.sync())
cases("Context.reset_run", one=lambda: a.reset_run())
cases("Context.get_means", one=lambda: a.get_means(), three=lambda: c.get_means())
cases("Context.energy", one=lambda: a.energy(), three=lambda: c.energy())
cases("Context.score", host=lambda: a.score(img()), host_bool=lambda: a.score(np.zeros((H, W), bool), True, 3.0), device=lambda: a.score(D1),
      device_some=lambda: a.score(D1, True, 0.0, STREAM))
cases("Context.get_trace", rows=lambda: c.get_trace(5), none=lambda: c.get_trace(0))
cases("Context.localized_means", all=lambda: c.localized_means(4), some=lambda: c.localized_means(4, ("c2", "a")))
cases("Context.set_edge_map", host=lambda: a.set_edge_map(np.zeros((H, W), np.uint16)), device=lambda: a.set_edge_map(D1), device_stream=lambda: a.set_edge_map(D1, STREAM),
      wrong_dtype=lambda: a.set_edge_map(np.zeros((H, W), np.int32)), wrong_kind=lambda: a.set_edge_map(1.5))
cases("Context.get_edge_map", host=lambda: a.get_edge_map(), device=lambda: a.get_edge_map(D1), device_stream=lambda: a.get_edge_map(D1, STREAM))
cases("Context.edge_map_from", one=lambda: a.edge_map_from(c, 4))
cases("Context.multiphase_labels_with", host=lambda: a.multiphase_labels_with(b), device=lambda: a.multiphase_labels_with(b, D1),
      device_stream=lambda: a.multiphase_labels_with(b, D1, STREAM))
cases("Context.get_stop_condition", one=lambda: a.get_stop_condition())
cases("Context.get_mask", default=lambda: a.get_mask(), inverted=lambda: a.get_mask(True))
cases("Context.components", all=lambda: a.components(), all_labels=lambda: a.components(8, True, D1, STREAM), cap=lambda: a.components(cap=2),
      cap_labels=lambda: a.components(8, True, D1, STREAM, 5), cap0=lambda: a.components(cap=0))
cases("Context.measure", all=lambda: a.measure(), all_some=lambda: a.measure(**CLEAN, stream=STREAM), cap=lambda: a.measure(cap=2), cap_some=lambda: a.measure(**CLEAN, cap=5, stream=STREAM),
      cap0=lambda: a.measure(cap=0))
cases("Context.overlaps", host_all=lambda: a.overlaps(np.zeros((H, W), np.int64)), host_cap=lambda: a.overlaps(np.zeros((H, W), np.int32), **CLEAN, cap=2),
      device_all=lambda: a.overlaps(D1), device_cap=lambda: a.overlaps(D1, **CLEAN, cap=6, stream=STREAM), device_cap0=lambda: a.overlaps(D1, cap=0))
cases("Context.contour_counts", default=lambda: a.contour_counts(), some=lambda: a.contour_counts(**CLEAN, simplify=False))
cases("Context.contours", default=lambda: a.contours(), some=lambda: a.contours(**CLEAN, simplify=False))
cases("Context.contours_subpixel", default=lambda: a.contours_subpixel(), some=lambda: a.contours_subpixel(**CLEAN))
cases("Context.get_mask_clean", default=lambda: a.get_mask_clean(), some=lambda: a.get_mask_clean(**CLEAN))
cases("Context.get_mask_clean_device", default=lambda: a.get_mask_clean_device(D1), some=lambda: a.get_mask_clean_device(D1, **CLEAN, stream=STREAM))
cases("Context.mask_morph", new=lambda: a.mask_morph("dilate", r2=4), filled=lambda: a.mask_morph(capi.MORPH_CLOSE, radius=2.5, **CLEAN, out=img()),
      device=lambda: a.mask_morph("open", 9, out=D1), device_some=lambda: a.mask_morph("erode", radius=1, **CLEAN, out=D1, stream=STREAM),
      both=lambda: a.mask_morph("erode", 1, 1.0), wrong=lambda: a.mask_morph("shrink", 1))
cases("Context.split", all=lambda: a.split(radius=3), all_labels=lambda: a.split(r2=9, **CLEAN, labels_ptr=D1, stream=STREAM), cap=lambda: a.split(radius=3, cap=2),
      cap_labels=lambda: a.split(9, None, **CLEAN, labels_ptr=D1, cap=5, stream=STREAM), cap0=lambda: a.split(radius=3, cap=0))
cases("Context.split_labels", default=lambda: a.split_labels(radius=3), some=lambda: a.split_labels(9, **CLEAN))
cases("Context.split_levelset", default=lambda: a.split_levelset(radius=3), some=lambda: a.split_levelset(9, None, **CLEAN, inside=2.0, outside=0.0))
cases("Context.morph_levelset", default=lambda: a.morph_levelset("open", radius=3), some=lambda: a.morph_levelset(0, 9, None, **CLEAN, inside=2.0, outside=0.0))
cases("Context.init_mask", host=lambda: a.init_mask(img()), host_bool=lambda: a.init_mask(np.zeros((H, W), bool), 2.0, 0.0), device=lambda: a.init_mask(D1),
      device_some=lambda: a.init_mask(D1, 2.0, 0.0, STREAM))
cases("Context.get_contour", one=lambda: a.get_contour())
cases("Context.separate", default=lambda: a.separate(np.zeros((H, W, 3), np.uint8)), inverted=lambda: a.separate(np.zeros((H, W, 3), np.int16), True))
cases("Context.perona_malik", default=lambda: a.perona_malik(), some=lambda: a.perona_malik(30, 0.2, 5))
cases("Context.last_run_ms", one=lambda: a.last_run_ms())
cases("Context.last_pm_ms", one=lambda: a.last_pm_ms())
cases("Context.launch_info", default=lambda: a.launch_info(), pm=lambda: a.launch_info(1))


def covered():
    """the public callables of capi that no case names (dataclasses, structs and the error type aside)"""
    text = open(__file__).read().split("def covered")[0].split("from chan_vese_amd import capi")[1]
    names = [n for n, v in vars(capi).items() if not n.startswith("_") and callable(v) and not isinstance(v, type)
             and getattr(v, "__module__", "").startswith("chan_vese_amd")]
    names += [f"Context.{n}" for n, v in vars(capi.Context).items() if not n.startswith("_") and callable(v)]
    return [n for n in names if not re.search(r"\b" + re.escape(n.split(".")[-1]) + r"\b", text)]


if __name__ == "__main__":
    run_cases(sys.stdout, "--full" in sys.argv[1:])
    sys.stdout.write(f"== not driven: {json.dumps(covered())}\n")
