"""Torch front end of the device-memory entry points: uint8 device tensors in, mask tensors out, nothing through host memory.

Import torch FIRST (this module does): torch ships its own libamdhip64 and the loader then shares that one HIP runtime with
libchanvese_hip.so -- the rule of capi.py.  No torch type crosses the C ABI: tensors are passed as `data_ptr()` addresses and the
current stream as its `cuda_stream` handle; the library orders its work against that stream with events and never synchronises it.
"""
import math

import torch

from . import capi


def _device_index(device):
    return device if isinstance(device, int) else (torch.device(device).index or 0)


def check_images(images, n, h, w, channels, device=0, layout=None):
    """Validates a batch of images for Segmenter.segment and returns its layout (capi.LAYOUT_PLANAR / LAYOUT_INTERLEAVED).
    ValueError for anything but a uint8 tensor of shape (N, H, W) [one channel], (N, C, H, W) or (N, H, W, C) on the CUDA/HIP device
    `device`, each member contiguous.  A shape that is both forms -- (N, 3, 3, 3): three channels of 3 x w or h x 3 pixels -- is taken
    as planar unless `layout` says otherwise; a `layout` the shape does not have is a ValueError.  Calls nothing in the library."""
    if not isinstance(images, torch.Tensor):
        raise ValueError(f"images must be a torch.Tensor, got {type(images).__name__}")
    if images.dtype != torch.uint8:
        raise ValueError(f"images must be uint8, got {images.dtype}")
    shape = tuple(images.shape)
    forms = []
    if (channels == 1 and shape == (n, h, w)) or shape == (n, channels, h, w):
        forms.append(capi.LAYOUT_PLANAR)
    if shape == (n, h, w, channels):
        forms.append(capi.LAYOUT_INTERLEAVED)
    if forms and layout is None:
        layout = forms[0]
    elif forms and layout in forms:
        pass
    elif forms:
        raise ValueError(f"images of shape {shape} do not have layout {layout!r}")
    else:
        raise ValueError(f"images of shape {shape} are neither ({n}, {channels}, {h}, {w}) nor ({n}, {h}, {w}, {channels})"
                         + (f" nor ({n}, {h}, {w})" if channels == 1 else ""))
    for i in range(n):
        if not images[i].is_contiguous():
            raise ValueError(f"images[{i}] is not contiguous (strides {tuple(images[i].stride())}): pitched sources are not supported")
    _check_device(images, device, "images")
    return layout


def check_levelsets(init, n, h, w, device=0):
    """Validates a tensor of initial level sets and returns its element width in bits (64 / 32).  ValueError otherwise."""
    if not isinstance(init, torch.Tensor):
        raise ValueError(f'init must be "checkerboard" or a torch.Tensor, got {init!r}')
    if init.dtype not in (torch.float64, torch.float32):
        raise ValueError(f"init must be float64 or float32, got {init.dtype}")
    if tuple(init.shape) != (n, h, w):
        raise ValueError(f"init of shape {tuple(init.shape)} is not ({n}, {h}, {w})")
    for i in range(n):
        if not init[i].is_contiguous():
            raise ValueError(f"init[{i}] is not contiguous")
    _check_device(init, device, "init")
    return 64 if init.dtype == torch.float64 else 32


def check_init(init, n, channels=1):
    """Validates a device-side start of Segmenter.segment and returns (kind, values): ("checkerboard", None), ("otsu", None),
    ("threshold", [t] * n), ("rect", [(x, y, w, h)] * n) or ("disk", [(cx, cy, r)] * n), every number an int.  A tuple's value is one
    entry for all members or a list of n.  ValueError for anything else.  Calls nothing in the library."""
    if isinstance(init, str):
        if init in ("checkerboard", "otsu"):
            return init, None
        raise ValueError(f'init must be "checkerboard", "otsu", a (kind, value) tuple or a tensor, got {init!r}')
    widths = {"threshold": 1, "rect": 4, "disk": 3}
    if not (isinstance(init, tuple) and len(init) == 2 and isinstance(init[0], str) and init[0] in widths):
        raise ValueError(f'init must be "checkerboard", "otsu", ("threshold", t), ("rect", (x, y, w, h)), ("disk", (cx, cy, r)) or a tensor, got {init!r}')
    kind, value = init
    width = widths[kind]

    def entry(v):
        if width == 1:
            ok = isinstance(v, int) and not isinstance(v, bool)
        else:
            ok = isinstance(v, (tuple, list)) and len(v) == width and all(isinstance(x, int) and not isinstance(x, bool) for x in v)
        if not ok:
            raise ValueError(f"init {kind!r}: {v!r} is not " + ("an int" if width == 1 else f"{width} ints"))
        return v if width == 1 else tuple(v)

    one = isinstance(value, int) if width == 1 else (isinstance(value, (tuple, list)) and len(value) == width and not isinstance(value[0], (tuple, list)))
    if one:
        rows = [entry(value)] * n
    elif isinstance(value, list):
        if len(value) != n:
            raise ValueError(f"init {kind!r}: {len(value)} entries for {n} members")
        rows = [entry(v) for v in value]
    else:
        raise ValueError(f"init {kind!r}: {value!r} is neither one entry nor a list of {n}")
    for r in rows:
        if kind == "threshold" and not 0 <= r <= 255 * channels:
            raise ValueError(f"init 'threshold': t must be in 0 .. {255 * channels}, got {r}")
        if kind == "rect" and (r[2] <= 0 or r[3] <= 0):
            raise ValueError(f"init 'rect': width and height must be positive, got {r}")
        if kind == "disk" and r[2] < 0:
            raise ValueError(f"init 'disk': the radius must not be negative, got {r}")
    return kind, rows


def check_levels(levels, h, w):
    """Validates Segmenter's `levels` and returns the pyramid's shapes, finest first (capi.pyramid_shapes).  ValueError for anything but
    an int >= 1 whose coarsest side stays at 16 or above.  Calls nothing in the library."""
    if not isinstance(levels, int) or isinstance(levels, bool):
        raise ValueError(f"levels must be an int, got {levels!r}")
    return capi.pyramid_shapes(h, w, levels)


def check_colour(colour, order, channels):
    """Validates Segmenter's `colour` and `order` and returns (colour, order) in lower case (colour None: no conversion).  ValueError for
    a space other than "ycrcb" / "yuv", an order other than "bgr" / "rgb", or a conversion of anything but 3 channels.  Calls nothing
    in the library."""
    capi.order_code(order)
    if colour is None:
        return None, order.lower()
    capi.colour_space_code(colour)
    if channels != 3:
        raise ValueError(f"colour={colour!r} converts three planes: channels must be 3, got {channels}")
    return colour.lower(), order.lower()


def _check_window(given, name, channels, what_codes, radius_of, radius_first=False):
    """(radius, codes, planes made) of Segmenter's `local` / `rank`: a name makes as many planes as are ingested, a tuple of 1 or 3 codes
    as many as it has; radius_of(radius, codes of the planes made) checks the radius, in front of the codes where it needs none."""
    if not isinstance(given, (tuple, list)) or len(given) != 2:
        raise ValueError(f"{name} must be (radius, what), got {given!r}")
    radius, what = given
    if radius_first:
        radius_of(radius, ())
    codes = what_codes(what)
    made = channels
    if not isinstance(what, str):
        if len(tuple(what)) not in (1, 3):
            raise ValueError(f"a tuple of {name} codes names 1 or 3 planes, got {what!r}")
        made = len(tuple(what))
    return radius_of(radius, codes[:made]), codes, made


def check_local(local, channels):
    """Validates Segmenter's `local` and returns (radius, codes, channels of the planes the run iterates on), or None for None.  `local`
    is (radius, what): what "mean" / "dev" (every plane; as many planes as are ingested), "stack" (copy, mean, deviation of ONE ingested
    plane: three planes) or a tuple of 1 or 3 capi.LOCAL_* codes (as many planes as codes).  ValueError for anything else.  Calls
    nothing in the library."""
    if local is None:
        return None
    radius, codes, made = _check_window(local, "local", channels, capi.local_what_codes, lambda r, _: capi.local_radius(r), radius_first=True)
    if isinstance(local[1], str) and local[1].lower() == "stack":
        if channels != 1:
            raise ValueError(f'local "stack" makes three planes of one: channels must be 1, got {channels}')
        made = 3
    return radius, codes, made


def check_rank(rank, channels):
    """Validates Segmenter's `rank` and returns (radius, codes, channels of the planes the filter makes), or None for None.  `rank` is
    (radius, what): what "min" / "max" / "median" / "open" / "close" / "tophat" / "bothat" (every plane; as many planes as are
    ingested) or a tuple of 1 or 3 capi.RANK_* codes (as many planes as codes).  A median binds the radius to
    capi.RANK_MEDIAN_RADIUS_MAX.  ValueError for anything else.  Calls nothing in the library."""
    return None if rank is None else _check_window(rank, "rank", channels, capi.rank_what_codes, capi.rank_radius)


def check_smooth(smooth, channels):
    """Validates Segmenter's `smooth` and returns ((radius, taps), codes, channels of the planes the stage makes), or None for None.
    `smooth` is (kernel, what): kernel a float sigma (the library's Gaussian, capi.gauss_taps) or a sequence of integer taps
    (capi.smooth_kernel); what "blur" / "detail" (every plane; as many planes as it is given) or a tuple of 1 or 3 capi.SMOOTH_* codes
    (as many planes as codes).  ValueError for anything else.  Only a Gaussian calls the library (a host function that needs no device)."""
    if smooth is None:
        return None
    return _check_window(smooth, "smooth", channels, capi.smooth_what_codes, lambda k, _: capi.smooth_kernel(k), radius_first=True)


def check_convex(convex):
    """Validates Segmenter's `convex` -- tau, (tau, sigma), or a dict of capi.make_convex_params' arguments but use_edge and resume -- and
    returns the dict, or None for None.  sigma defaults to 1 / (8 tau)."""
    if convex is None:
        return None
    if isinstance(convex, dict):
        out = dict(convex)
        if set(out) - {"tau", "sigma", "stop_rms", "means_every"}:
            raise ValueError(f"convex: unknown keys {sorted(set(out) - {'tau', 'sigma', 'stop_rms', 'means_every'})} (tau, sigma, stop_rms, means_every)")
    elif isinstance(convex, tuple) and len(convex) == 2:
        out = dict(tau=convex[0], sigma=convex[1])
    else:
        out = dict(tau=convex)
    tau, sigma = out.get("tau", 0.25), out.get("sigma")
    for name, x in (("tau", tau), ("sigma", sigma)):
        if x is None and name == "sigma":
            continue
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) or x <= 0:
            raise ValueError(f"convex must be None, tau, (tau, sigma) or a dict with finite steps > 0, got {name} = {x!r}")
    if sigma is not None and 8.0 * tau * sigma > 1.0:
        raise ValueError(f"convex: 8 tau sigma must not exceed 1, got tau = {tau!r}, sigma = {sigma!r}")
    return out


def check_edge_sigma(edge_sigma, edge):
    """Validates Segmenter's `edge_sigma` and returns its (radius, taps), or None for None.  It needs edge=K."""
    if edge_sigma is None:
        return None
    if edge is None:
        raise ValueError("edge_sigma= needs edge=K: it blurs the planes the edge map is built from")
    if isinstance(edge_sigma, bool) or not isinstance(edge_sigma, (int, float)) or not math.isfinite(edge_sigma) or not 0 < edge_sigma <= 21:
        raise ValueError(f"edge_sigma must be None or a finite sigma in (0, 21], got {edge_sigma!r}")
    return capi.gauss_taps(float(edge_sigma))


def scale_init(kind, rows, levels):
    """The numbers of a ("rect", ..) / ("disk", ..) start, given in finest pixels, on the coarsest of `levels` levels: every number is
    shifted right by levels - 1 (an arithmetic shift: negative coordinates round down).  Other kinds pass through."""
    if kind not in ("rect", "disk") or levels == 1:
        return rows
    return [tuple(v >> (levels - 1) for v in r) for r in rows]


def _check_device(t, device, name):
    if t.device.type != "cuda" or (t.device.index or 0) != device:
        raise ValueError(f"{name} lives on {t.device}, the contexts on cuda:{device}")


class Segmenter:
    """N contexts of one shape on one GPU, kept for the object's lifetime (cvh_create allocates: a stream of frames reuses them).
    levels = L > 1 makes every member a pyramid of L contexts (capi.pyramid_shapes; N x L contexts in all, `pyramids[i]` finest first,
    `contexts` the finest ones) and segment() a coarse-to-fine run; every level takes `params` and `options` as given, nothing is
    rescaled.  levels = 1 is the plain path, call for call.
    colour = "ycrcb" / "yuv" (three channels only) makes segment() convert the planes, read as (R, G, B) or (B, G, R) by `order`, into
    (Y, Cr, Cb) / (Y, U, V) on the device (cvh_convert_colour_batch): params.lambda1[0] / lambda2[0] then weigh the luma.  None (the
    default) converts nothing.
    local = (radius, what) makes the run iterate on local statistics of the ingested planes (check_local; cvh_local_planes_batch): the
    N members ingest into `sources`, contexts of `channels` channels of their own, and `contexts` -- the ones that iterate, `run_channels`
    channels, which `params`, `options` and every other method refer to -- receive the local planes.  None (the default): `contexts`
    ingest themselves.
    rank = (radius, what) makes the run iterate on rank planes of the ingested planes -- a median against impulse noise, a top-hat
    against a shading ramp (check_rank; cvh_rank_planes_batch) -- in source contexts of its own, as local= does.  With both given the
    rank filter runs FIRST, into `ranked`, contexts of the filter's channels, and local= works on its result.
    smooth = (kernel, what) makes the run iterate on smoothed planes -- the blur under a Gaussian of sigma `kernel` (a float) or under the
    integer taps given, or the detail the blur leaves (check_smooth; cvh_smooth_planes_batch) -- in source contexts of its own, as rank=
    does, and is accepted and refused where rank= is.  The stages run colour -> rank -> smooth -> local; a stage that another follows
    writes into contexts of its own (`ranked`, `smoothed`).
    phases = 4 (include/chanvese_hip.h, "Four phases") makes every member a PAIR of contexts, `contexts[i]` holding phi1 and `contexts_b[i]`
    phi2, both fed the same device tensor; segment() then iterates the pairs (cvh_multiphase_run_batch) and returns labels 0 .. 3, phase_masks()
    gives the two mask tensors, and the post-processing methods take phase = 0 | 1.  It needs levels = 1 and neither local= nor rank=.
    phases = 2 (the default) is the plain path, call for call.
    localized = R (1 .. 127; include/chanvese_hip.h, "Localised regions") makes the members run cvh_localized_run_batch -- region means over
    the (2 R + 1)^2 window of every pixel -- instead of the two-phase run, from whatever init= gives; everything after the run is
    unchanged.  The local force is small: start near the object (init="otsu", a rect, a disk, a mask) and raise mu.  It needs phases = 2
    and levels = 1, and segment() refuses energy_every and reinit_every with it.  None (the default) is the plain path, call for call.
    edge = K (finite, > 0; include/chanvese_hip.h, "Edge-weighted length") makes segment() build every member's edge plane from its own
    planes as they stand after the preprocessing above (cvh_edge_map_batch with that K) and iterate with cvh_geodesic_run_batch -- the
    length term weighted by the plane -- instead of the two-phase run; edge_maps() returns the planes.  It needs phases = 2, levels = 1 and
    no localized=, and segment() refuses energy_every and reinit_every with it.  None (the default) is the plain path, call for call.
    convex = tau, (tau, sigma) or a dict of tau, sigma, stop_rms, means_every (include/chanvese_hip.h, "Convex relaxation"; sigma defaults
    to 1 / (8 tau), stop_rms to 0, means_every to 1) makes segment() run the primal-dual iteration of the convex relaxation from the mask
    of the start (cvh_convex_run_batch) instead of a level-set descent: the result does not depend on the start for fixed means.  With
    edge=K it runs the weighted model on the edge planes the map stage builds; relaxed() returns v.  It needs phases = 2, levels = 1 and
    no localized=; reinit_every and energy_every are refused.
    edge_sigma = sigma (0 < sigma <= 21; needs edge=K) builds the edge plane from G_sigma * I, the textbook edge function: every member's
    planes, as the preprocessing left them, are blurred into scratch contexts (`edge_sources`; cvh_smooth_planes_batch) and
    cvh_edge_map_batch takes those as its sources, while the run iterates on the unblurred planes.  None: the map is built from the
    planes themselves."""
    levels = 1
    phases = 2
    localized = None
    edge = None
    convex = None
    contexts_b = ()
    colour = None
    local = None
    rank = None
    smooth = None
    edge_kernel = None
    sources = ()
    ranked = ()
    smoothed = ()
    edge_sources = ()

    @property
    def run_channels(self):
        """channels of the planes the run iterates on: the ingested ones', or with rank=, smooth= and local= what their codes make of them"""
        return self.local[2] if self.local else self.smooth[2] if self.smooth else self.rank[2] if self.rank else self.channels

    def __init__(self, n, h, w, channels=1, params=None, device=0, options=None, levels=1, colour=None, order="rgb", local=None, rank=None,
                 phases=2, params2=None, localized=None, edge=None, smooth=None, edge_sigma=None, convex=None):
        if n < 1:
            raise ValueError(f"n must be >= 1, got {n}")
        self.convex = check_convex(convex)
        if self.convex is not None and (phases == 4 or levels != 1 or localized is not None):
            raise ValueError("convex= needs phases = 2, levels = 1 and no localized=: the relaxation iterates one function v on one level")
        if edge is not None:
            if isinstance(edge, bool) or not isinstance(edge, (int, float)) or not math.isfinite(edge) or edge <= 0:
                raise ValueError(f"edge must be None or a finite K > 0, got {edge!r}")
            if phases == 4 or levels != 1 or localized is not None:
                raise ValueError("edge= needs phases = 2, levels = 1 and no localized=: the edge-weighted run iterates one level set on one level")
        if localized is not None:
            if not isinstance(localized, int) or isinstance(localized, bool) or not 1 <= localized <= 127:
                raise ValueError(f"localized must be None or a window radius 1 .. 127, got {localized!r}")
            if phases == 4 or levels != 1:
                raise ValueError("localized= needs phases = 2 and levels = 1: the localised run iterates one level set on one level")
        if phases not in (2, 4) or isinstance(phases, bool):
            raise ValueError(f"phases must be 2 or 4, got {phases!r}")
        if phases == 4 and (levels != 1 or local is not None or rank is not None):
            raise ValueError("phases=4 needs levels = 1 and neither local= nor rank=")
        if phases == 4 and smooth is not None:
            raise ValueError("phases=4 needs levels = 1 and none of local=, rank= and smooth=")
        if phases != 4 and params2 is not None:
            raise ValueError("params2 (the parameters of the second level set) needs phases=4")
        shapes = check_levels(levels, h, w)
        self.colour, self.order = check_colour(colour, order, channels)
        self.rank = check_rank(rank, channels)
        self.smooth = check_smooth(smooth, self.rank[2] if self.rank else channels)
        self.local = check_local(local, self.smooth[2] if self.smooth else self.rank[2] if self.rank else channels)
        self.edge_kernel = check_edge_sigma(edge_sigma, edge)
        self.n, self.h, self.w, self.channels, self.levels = n, h, w, channels, levels
        self.sources = []
        self.ranked = []
        self.smoothed = []
        self.edge_sources = []
        self.device = _device_index(device)
        self.thresholds = None   # Otsu's thresholds of the last segment(init="otsu")
        self.level_steps = None  # levels > 1: the iterations of the last segment() per member and level, finest first
        self.energy_series = None   # segment(energy_every=K > 0): [(iterations so far, capi.Energy)] of the last segment() per member
        self.contexts = []
        self.pyramids = []
        self.phases = phases
        self.localized = localized
        self.edge = None if edge is None else float(edge)
        self.contexts_b = []
        try:
            for _ in range(n if phases == 4 else 0):   # the second level sets: params2 (None: params), the same options
                ctx = capi.Context(h, w, channels, params2 if params2 is not None else params, self.device)
                self.contexts_b.append(ctx)
                for key, value in (options or {}).items():
                    ctx.set_option(key, value)
            for _ in range(n):
                self.pyramids.append([])
                for k, (lh, lw) in enumerate(shapes):
                    ctx = capi.Context(lh, lw, self.run_channels, params, self.device)
                    self.pyramids[-1].append(ctx)
                    if k == 0:
                        self.contexts.append(ctx)
                    for key, value in (options or {}).items():
                        ctx.set_option(key, value)
                if self.local or self.rank or self.smooth:
                    self.sources.append(capi.Context(h, w, channels, None, self.device))
                if self.rank and (self.local or self.smooth):
                    self.ranked.append(capi.Context(h, w, self.rank[2], None, self.device))
                if self.smooth and self.local:
                    self.smoothed.append(capi.Context(h, w, self.smooth[2], None, self.device))
                if self.edge_kernel:
                    self.edge_sources.append(capi.Context(h, w, self.run_channels, None, self.device))
        except Exception:
            self.close()
            raise

    def close(self):
        for pyr in self.pyramids:
            for ctx in pyr:
                ctx.close()
        for ctx in list(self.sources) + list(self.ranked) + list(self.smoothed) + list(self.edge_sources) + list(self.contexts_b):
            ctx.close()
        self.smoothed = []
        self.edge_sources = []
        self.contexts_b = []
        self.contexts = []
        self.pyramids = []
        self.sources = []
        self.ranked = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _phase(self, phase):
        """the contexts a post-processing method works on: phase 0 the first level sets (all there are with phases = 2), 1 the second"""
        if phase not in (0, 1) or isinstance(phase, bool) or (phase == 1 and self.phases != 4):
            raise ValueError(f"phase must be 0" + (" or 1" if self.phases == 4 else " (phases = 2: there is one level set)") + f", got {phase!r}")
        return self.contexts_b if phase == 1 else self.contexts

    def _start(self, contexts, kind, start, init, bits, stream):
        """the initial level sets of `contexts` (phases = 4: of either phase), as segment() builds them"""
        if kind == "checkerboard":
            capi.init_checkerboard_batch(contexts)
        elif kind == "otsu":
            return capi.init_otsu_batch(contexts)
        elif kind == "threshold":
            capi.init_threshold_batch(contexts, start)
        elif kind == "rect":
            capi.init_rect_batch(contexts, start)
        elif kind == "disk":
            capi.init_disk_batch(contexts, start)
        else:
            for i, ctx in enumerate(contexts):
                ctx.set_levelset_device(init[i].data_ptr(), bits, stream)
        return None

    def _segment4(self, images, max_steps, perona_malik, init, init2, layout):
        """segment() with phases = 4: ingest into both contexts of every pair -> (Perona-Malik, colour on both) -> phi1 from init, phi2 from
        init2 -> cvh_multiphase_run_batch (all pairs in shared launches) -> labels.  Returns (labels, steps, norms): labels a uint8 tensor (N, H, W) of 0 .. 3 =
        mask(phi1) + 2 mask(phi2), steps the iterations and norms the (||d1||, ||d2||) of every pair."""
        kinds = []
        for name, given in (("init", init), ("init2", init2)):
            if isinstance(given, tuple) and len(given) == 2 and given[0] == "mask":
                raise ValueError(f"{name}: a mask start is not built with phases=4")
            kinds.append(check_init(given, self.n, self.channels) if isinstance(given, (str, tuple)) else (None, None))
        layout = check_images(images, self.n, self.h, self.w, self.channels, self.device, layout)
        bits = [None if k[0] is not None else check_levelsets(g, self.n, self.h, self.w, self.device) for k, g in zip(kinds, (init, init2))]
        if perona_malik is not None and len(perona_malik) != 3:
            raise ValueError("perona_malik must be (K, L, T)")
        stream = self._stream()
        both = list(self.contexts) + list(self.contexts_b)
        capi.set_image_device_batch(both, [images[i].data_ptr() for i in range(self.n)] * 2, layout, stream)
        if perona_malik is not None:
            capi.perona_malik_batch(both, *perona_malik)
        if self.colour is not None:
            capi.convert_colour_batch(both, self.colour, self.order)
        th = self._start(self.contexts, kinds[0][0], kinds[0][1], init, bits[0], stream)
        if th is not None:
            self.thresholds = th
        self._start(self.contexts_b, kinds[1][0], kinds[1][1], init2, bits[1], stream)
        res = capi.multiphase_run_batch(list(zip(self.contexts, self.contexts_b)), max_steps)
        labels = torch.empty((self.n, self.h, self.w), dtype=torch.uint8, device=images.device)
        for i, (a, b) in enumerate(zip(self.contexts, self.contexts_b)):
            a.multiphase_labels_with(b, labels[i].data_ptr(), stream)
        return labels, [r[0] for r in res], [r[1] for r in res]

    def default_init2(self):
        """the default start of the second level sets: the checkerboard of cvh_levelset_checkerboard_host rolled by (2, 3) pixels (two
        identical starts stay identical forever), as a float64 device tensor (N, H, W)"""
        one = torch.from_numpy(capi.checkerboard_host(self.h, self.w)).roll((2, 3), dims=(0, 1))
        return one.to(torch.device("cuda", self.device)).unsqueeze(0).repeat(self.n, 1, 1).contiguous()

    def phase_masks(self, invert=False):
        """phases = 4: the masks of the two level sets, two uint8 tensors (N, H, W); labels = masks[0] + 2 masks[1] (invert = False)"""
        if self.phases != 4:
            raise ValueError("phase_masks needs phases=4")
        out = []
        for contexts in (self.contexts, self.contexts_b):
            masks = torch.empty((self.n, self.h, self.w), dtype=torch.uint8, device=torch.device("cuda", self.device))
            capi.get_mask_device_batch(contexts, [masks[i].data_ptr() for i in range(self.n)], invert, self._stream())
            out.append(masks)
        return tuple(out)

    def segment(self, images, max_steps=-1, perona_malik=None, init="checkerboard", invert=False, layout=None, reinit_every=0, energy_every=0,
                init2=None):
        """ingest -> (Perona-Malik batch) -> initial level set -> cvh_run_batch -> masks.  Returns (masks, steps, norms): masks a uint8
        tensor (N, H, W) on the images' device, valid for the next operation on the current stream without a host wait of the caller's;
        steps / norms the iterations and the last ||u_diff|| of every member.  `layout` (capi.LAYOUT_*) is needed only for a shape that is
        both planar and interleaved (check_images).  reinit_every = K > 0 runs segments of K iterations with a reinitialisation of the
        members still iterating between segments (capi.run_batch_with_reinit; max_steps stays the total budget); 0 is one cvh_run_batch.
        init: "checkerboard"; a float64 / float32 tensor (N, H, W); or a start built on the device from the (smoothed) planes or from
        numbers -- "otsu" (+1 above Otsu's threshold of the grey values, -1 elsewhere; self.thresholds then holds the N thresholds),
        ("threshold", t), ("rect", (x, y, w, h)) and ("disk", (cx, cy, r)) (1 inside, 0 outside), the tuple's value one entry for all
        members or a list of N (check_init); or ("mask", t), t a uint8 or bool device tensor (N, H, W): +1 where it is nonzero, -1 elsewhere,
        written on the device at a byte per pixel (cvh_init_mask_device_batch) -- a network's prediction, the previous frame's masks,
        clean_masks' output.  A text or tuple `init` is validated first, before the images; a tensor `init`, or a mask's tensor, after them.
        levels > 1: ingest -> (Perona-Malik batch on the finest level) -> restrict batches downwards -> the start on the COARSEST level ->
        per level run_batch and a prolong batch (capi.run_coarse_to_fine_batch; max_steps applies per level) -> masks from the finest.
        "otsu" and ("threshold", t) act on the coarsest planes; the numbers of "rect" and "disk" are given in finest pixels and shifted
        right by levels - 1 (scale_init).  steps / norms are the finest level's, self.level_steps holds every level's counts.  A tensor
        `init`, a ("mask", t) init (a mask is not resampled through the pyramid) and reinit_every > 0 are ValueErrors with levels > 1.
        colour (the constructor's): all members are converted with ONE cvh_convert_colour_batch AFTER the Perona-Malik batch, if any, and
        BEFORE the start and the run (with levels > 1: on the finest level, before the restricts -- a restrict of converted planes is just
        a restrict).  "otsu" and ("threshold", t) therefore see the CONVERTED planes (g = Y + the two chroma bytes), and images() returns
        them.
        local (the constructor's): the images are ingested, smoothed and converted in `sources`; ONE cvh_local_planes_batch then writes the
        planes the run iterates on into `contexts`, BEFORE the restricts, the start and the run.  "otsu" and ("threshold", t) see the
        LOCAL planes, and images() returns them; masks come out as before.
        rank (the constructor's): as local, with ONE cvh_rank_planes_batch; "otsu" and ("threshold", t) see the RANK planes.  With both,
        the rank call writes into `ranked` and the local call reads from there.
        smooth (the constructor's): as rank, with ONE cvh_smooth_planes_batch behind the rank call and in front of the local call; "otsu"
        and ("threshold", t) see the SMOOTHED planes.  edge_sigma (the constructor's): ONE more cvh_smooth_planes_batch blurs the planes
        the run iterates on into `edge_sources`, from which cvh_edge_map_batch builds the edge planes.
        energy_every = K > 0 runs segments of K iterations with the energy of the members still iterating taken after each
        (capi.run_batch_monitored, one cvh_energy_batch per segment; max_steps stays the total budget) and stores the series in
        self.energy_series; 0 takes none and leaves self.energy_series None.  It is a ValueError with levels > 1 or reinit_every > 0.
        energies() gives the terms of the final level sets either way.
        phases = 4 (the constructor's): phi1 starts as `init` says, phi2 as `init2` does -- the same forms but a mask; None: the checkerboard
        rolled by (2, 3) pixels (default_init2) -- and the result is (labels, steps, norms) of _segment4; invert, reinit_every and
        energy_every are ValueErrors there."""
        if self.phases == 4:
            if invert or reinit_every or energy_every:
                raise ValueError("phases=4: invert, reinit_every and energy_every are not built for a pair of level sets")
            return self._segment4(images, max_steps, perona_malik, init, self.default_init2() if init2 is None else init2, layout)
        if init2 is not None:
            raise ValueError("init2 (the start of the second level set) needs phases=4")
        if self.localized is not None and (reinit_every or energy_every):
            raise ValueError("localized=: reinit_every and energy_every are not built for the localised run")
        if self.edge is not None and (reinit_every or energy_every):
            raise ValueError("edge=: reinit_every and energy_every are not built for the edge-weighted run")
        if self.convex is not None and (reinit_every or energy_every):
            raise ValueError("convex=: reinit_every and energy_every are not built for the relaxation (it has no level set to reinitialise)")
        kind, bits = None, None
        mask_init = isinstance(init, tuple) and len(init) == 2 and init[0] == "mask"
        if mask_init and self.levels > 1:
            raise ValueError("a mask init needs levels = 1: a mask is not resampled through the pyramid")
        if self.levels > 1:
            if not isinstance(init, (str, tuple)):
                raise ValueError("a tensor init needs levels = 1: with levels > 1 the start is built on the coarsest level")
            if reinit_every:
                raise ValueError("reinit_every needs levels = 1")
            if energy_every:
                raise ValueError("energy_every needs levels = 1")
        if not isinstance(energy_every, int) or isinstance(energy_every, bool) or energy_every < 0:
            raise ValueError(f"energy_every must be an int >= 0, got {energy_every!r}")
        if energy_every and reinit_every:
            raise ValueError("energy_every and reinit_every cannot be combined: a reinitialisation replaces the level set the series follows")
        if mask_init:
            kind = "mask"
        elif isinstance(init, (str, tuple)):
            kind, start = check_init(init, self.n, self.run_channels)
        layout = check_images(images, self.n, self.h, self.w, self.channels, self.device, layout)
        if mask_init:
            start = self._byte_planes(init[1], "the mask of init")
        elif kind is None:
            bits = check_levelsets(init, self.n, self.h, self.w, self.device)
        if perona_malik is not None and len(perona_malik) != 3:
            raise ValueError("perona_malik must be (K, L, T)")
        stream = self._stream()
        self.energy_series = None
        ingested = self.sources if (self.local or self.rank or self.smooth) else self.contexts
        capi.set_image_device_batch(ingested, [images[i].data_ptr() for i in range(self.n)], layout, stream)
        if perona_malik is not None:
            K, L, T = perona_malik
            capi.perona_malik_batch(ingested, K, L, T)
        if self.colour is not None:
            capi.convert_colour_batch(ingested, self.colour, self.order)
        made = self.sources   # where the last stage has left the planes
        if self.rank:
            capi.rank_planes_batch(made, self.ranked or self.contexts, self.rank[0], self.rank[1])
            made = self.ranked
        if self.smooth:
            capi.smooth_planes_batch(made, self.smoothed or self.contexts, [int(t) for t in self.smooth[0][1]], self.smooth[1])
            made = self.smoothed
        if self.local:
            capi.local_planes_batch(made, self.contexts, self.local[0], self.local[1])
        first = self.contexts   # the level the start is built on
        if self.levels > 1:
            for k in range(self.levels - 1):
                capi.restrict_image_batch([p[k] for p in self.pyramids], [p[k + 1] for p in self.pyramids])
            first = [p[-1] for p in self.pyramids]
            start = scale_init(kind, start, self.levels)
        if kind == "checkerboard":
            capi.init_checkerboard_batch(first)
        elif kind == "otsu":
            self.thresholds = capi.init_otsu_batch(first)
        elif kind == "threshold":
            capi.init_threshold_batch(first, start)
        elif kind == "rect":
            capi.init_rect_batch(first, start)
        elif kind == "disk":
            capi.init_disk_batch(first, start)
        elif kind == "mask":
            capi.init_mask_batch(first, [start[i].data_ptr() for i in range(self.n)], 1.0, -1.0, stream)
        else:
            for i, ctx in enumerate(self.contexts):
                ctx.set_levelset_device(init[i].data_ptr(), bits, stream)
        if self.levels > 1:
            per_level = capi.run_coarse_to_fine_batch(self.pyramids, max_steps)
            self.level_steps = [[r[0] for r in member] for member in per_level]
            res = [member[0] for member in per_level]
        elif energy_every:
            mon = capi.run_batch_monitored(self.contexts, max_steps, energy_every)
            self.energy_series = [m[2] for m in mon]
            res = [m[:2] for m in mon]
        elif self.localized is not None:
            res = [r[:2] for r in capi.localized_run_batch(self.contexts, self.localized, max_steps)]
        elif self.edge is not None:   # (the planes the run iterates on, as every stage above has left them)
            if self.edge_kernel:   # g from G_sigma * I; the run keeps the unblurred planes
                capi.smooth_planes_batch(self.contexts, self.edge_sources, [int(t) for t in self.edge_kernel[1]], "blur")
            capi.edge_map_batch(self.contexts, self.edge_sources or self.contexts, self.edge)
            if self.convex is not None:   # the weighted relaxation: rho = mu g
                res = [r[:2] for r in capi.convex_run_batch(self.contexts, max_steps, dict(self.convex, use_edge=True))]
            else:
                res = [r[:2] for r in capi.geodesic_run_batch(self.contexts, max_steps)]
        elif self.convex is not None:
            res = [r[:2] for r in capi.convex_run_batch(self.contexts, max_steps, self.convex)]
        else:
            res = capi.run_batch_with_reinit(self.contexts, max_steps, reinit_every)
        masks = torch.empty((self.n, self.h, self.w), dtype=torch.uint8, device=images.device)
        capi.get_mask_device_batch(self.contexts, [masks[i].data_ptr() for i in range(self.n)], invert, stream)
        return masks, [r[0] for r in res], [r[1] for r in res]

    def relaxed(self):
        """convex=: the members' relaxed functions v as the last segment() left them, a float64 device tensor (N, H, W) with values in
        [0, 1] (cvh_get_relaxed_device), valid for the next operation on the current stream; the masks are v > 1/2."""
        if self.convex is None:
            raise ValueError("relaxed needs convex=")
        out = torch.empty((self.n, self.h, self.w), dtype=torch.float64, device=torch.device("cuda", self.device))
        for i, ctx in enumerate(self.contexts):
            ctx.relaxed(ptr=out[i].data_ptr(), stream=self._stream())
        return out

    def edge_maps(self):
        """edge=: the members' edge planes as the last segment() built them, a uint16 device tensor (N, H, W), g = value / 32768
        (cvh_get_edge_map_device), valid for the next operation on the current stream."""
        if self.edge is None:
            raise ValueError("edge_maps needs edge=K")
        out = torch.empty((self.n, self.h, self.w), dtype=torch.uint16, device=torch.device("cuda", self.device))
        for i, ctx in enumerate(self.contexts):
            ctx.get_edge_map(out[i].data_ptr(), self._stream())
        return out

    def energies(self):
        """The Chan-Sandberg-Vese functional of every member's current level set -- after segment(): the final ones --, term by term
        (cvh_energy_batch: one set of launches, one host wait).  Returns [capi.Energy], each bit for bit its context's Context.energy()."""
        return capi.energy_batch(self.contexts)

    def score(self, truths, invert=False, tol=2.0, phase=0):
        """Every member's mask against its ground truth (cvh_score_mask_device_batch: one set of launches on the device, one host wait):
        truths is a uint8 or bool device tensor (N, H, W), non-zero = foreground (a bool tensor is viewed as uint8, no copy), ordered
        behind the current stream; tol the surface tolerance in pixels.  Returns [capi.Score], each integer its context's Context.score()."""
        if not isinstance(truths, torch.Tensor) or truths.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"truths must be a uint8 or bool tensor, got {getattr(truths, 'dtype', type(truths))}")
        if tuple(truths.shape) != (self.n, self.h, self.w):
            raise ValueError(f"truths must have shape {(self.n, self.h, self.w)}, got {tuple(truths.shape)}")
        _check_device(truths, self.device, "truths")
        t = truths.view(torch.uint8) if truths.dtype == torch.bool else truths
        if not t.is_contiguous():
            t = t.contiguous()
        return capi.score_batch(self._phase(phase), [t[i].data_ptr() for i in range(self.n)], invert, tol, self._stream())

    def components(self, conn=4, invert=False, phase=0):
        """The connected components of every member's mask (cvh_components_batch): (labels, counts), labels an int32 tensor (N, H, W) --
        0 background, 1..K in the order of scipy.ndimage.label -- valid for the next operation on the current stream, counts the K of
        every member.  One host wait, for the counts."""
        labels = torch.empty((self.n, self.h, self.w), dtype=torch.int32, device=torch.device("cuda", self.device))
        counts = capi.components_batch(self._phase(phase), [labels[i].data_ptr() for i in range(self.n)], conn, invert, self._stream())
        return labels, counts

    def _byte_planes(self, t, name):
        """a uint8 or bool device tensor (N, H, W) as contiguous uint8 (a bool tensor is viewed, no copy); ValueError for anything else"""
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.uint8, torch.bool):
            raise ValueError(f"{name} must be a uint8 or bool tensor, got {getattr(t, 'dtype', type(t))}")
        if tuple(t.shape) != (self.n, self.h, self.w):
            raise ValueError(f"{name} must have shape {(self.n, self.h, self.w)}, got {tuple(t.shape)}")
        _check_device(t, self.device, name)
        t = t.view(torch.uint8) if t.dtype == torch.bool else t
        return t if t.is_contiguous() else t.contiguous()

    def clean_masks(self, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, morph=None, radius=0.0, phase=0):
        """Every member's cleaned mask (cvh_get_mask_clean_device_batch; Context.get_mask_clean names the steps) as a uint8 tensor
        (N, H, W), valid for the next operation on the current stream without a host wait of the caller's.  morph = "dilate" / "erode" /
        "open" / "close" (or a capi.MORPH_* code) applies that operation by a disk of `radius` pixels (one number or one per member) behind
        the cleaning (cvh_get_mask_morph_device_batch: one set of launches); None is the cleaned mask alone."""
        masks = torch.empty((self.n, self.h, self.w), dtype=torch.uint8, device=torch.device("cuda", self.device))
        ptrs = [masks[i].data_ptr() for i in range(self.n)]
        if morph is None:
            capi.get_mask_clean_device_batch(self._phase(phase), ptrs, conn, invert, min_area, fill_holes, keep_largest, self._stream())
        else:
            capi.mask_morph_batch(self._phase(phase), ptrs, morph, radius=radius, conn=conn, invert=invert, min_area=min_area, fill_holes=fill_holes,
                                  keep_largest=keep_largest, stream=self._stream())
        return masks

    def morph(self, op, radius, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, inside=1.0, outside=-1.0, phase=0):
        """clean_masks(morph=op, radius=radius) IN PLACE (cvh_morph_levelset_batch: one set of launches, one host wait): every member's
        level set becomes `inside` where that mask is 1 and `outside` elsewhere, and a new run begins as after a fresh level set.
        components(), measure(), contours(), score(), levelsets() and further iterations then see the result; the masks never leave the
        device.  op None bakes the cleaned mask in."""
        capi.morph_levelset_batch(self._phase(phase), op, radius=radius, conn=conn, invert=invert, min_area=min_area, fill_holes=fill_holes,
                                  keep_largest=keep_largest, inside=inside, outside=outside)

    def split(self, radius, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, phase=0):
        """Touching objects taken apart (cvh_split_batch, "Object split" in include/chanvese_hip.h): every member's cleaned mask eroded by
        a disk of `radius` pixels (one number or one per member), its cores labelled and grown back inside the mask.  Returns
        (labels, counts): labels an int32 tensor (N, H, W) -- 0 background, 1..K one label per core, cut pixels included -- valid for the
        next operation on the current stream, counts the K of every member.  Only reads."""
        labels = torch.empty((self.n, self.h, self.w), dtype=torch.int32, device=torch.device("cuda", self.device))
        counts = capi.split_batch(self._phase(phase), [labels[i].data_ptr() for i in range(self.n)], radius=radius, conn=conn, invert=invert,
                                  min_area=min_area, fill_holes=fill_holes, keep_largest=keep_largest, stream=self._stream())
        return labels, counts

    def split_levelset(self, radius, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, inside=1.0, outside=-1.0, phase=0):
        """split() IN PLACE (cvh_split_levelset_batch): every member's level set becomes `inside` on the split objects and `outside` on the
        one-pixel cut lines and the background, and a new run begins as after a fresh level set.  components(), measure(), contours(),
        overlaps(), match() and further iterations then see the split objects."""
        capi.split_levelset_batch(self._phase(phase), radius=radius, conn=conn, invert=invert, min_area=min_area, fill_holes=fill_holes,
                                  keep_largest=keep_largest, inside=inside, outside=outside)

    def measure(self, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, cap=None, phase=0):
        """The components of every member's mask -- clean_masks' for the same options, (0, 0, False) the raw one -- measured on the device
        (cvh_measure_batch: one set of launches, ordered behind the current stream): one (K, table) per member, table a numpy structured
        array (capi.REGION_DTYPE) of the first min(K, cap) rows, bit for bit its context's Context.measure(); capi.region_shapes derives
        centroid, moments, axes, mean and variance from it.  cap = None asks for every row at the price of a first call for the counts."""
        return capi.measure_batch(self._phase(phase), conn, invert, min_area, fill_holes, keep_largest, cap, self._stream())

    def _label_planes(self, labels):
        """an int32 device tensor (N, H, W), or a list of N tensors (H, W), as N contiguous planes; ValueError for anything else"""
        planes = list(labels) if not isinstance(labels, torch.Tensor) else ([labels[i] for i in range(labels.shape[0])] if labels.dim() == 3 else None)
        if planes is None or len(planes) != self.n:
            raise ValueError(f"labels must be an int32 tensor of shape {(self.n, self.h, self.w)} or a list of {self.n} tensors")
        out = []
        for i, p in enumerate(planes):
            if not isinstance(p, torch.Tensor) or p.dtype != torch.int32 or tuple(p.shape) != (self.h, self.w):
                raise ValueError(f"labels[{i}] must be an int32 tensor of shape {(self.h, self.w)}, got {getattr(p, 'dtype', type(p))} "
                                 f"{tuple(getattr(p, 'shape', ()))}")
            _check_device(p, self.device, f"labels[{i}]")
            out.append(p if p.is_contiguous() else p.contiguous())
        return out

    def overlaps(self, labels, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, cap=None, phase=0):
        """The contingency table of every member's components -- measure's for the same options -- against a second label plane each
        (cvh_overlaps_device_batch: one set of launches, ordered behind the current stream).  labels is an int32 device tensor
        (N, H, W) or a list of N tensors (H, W): an instance ground truth, or the tensors components() returned for the PREVIOUS FRAME
        (frame-to-frame correspondence: the labels never leave the device).  Returns one row array per member (capi.OVERLAP_DTYPE: a, b,
        count; sorted by a, then b; a = 0 and b = 0 included), byte for byte its context's Context.overlaps()."""
        planes = self._label_planes(labels)
        res = capi.overlaps_batch(self._phase(phase), [p.data_ptr() for p in planes], conn, invert, min_area, fill_holes, keep_largest, cap, self._stream())
        return [rows for rows, _ in res]

    def match(self, labels, threshold=0.5, conn=4, invert=False, min_area=0, fill_holes=0, keep_largest=False, phase=0):
        """overlaps() read as object-level scores (capi.match_overlaps on every member's table): one (score, match_of_a, ious) per member
        -- score a capi.ObjectScore at the IoU threshold (strictly above; a number >= 0.5 taken in thousandths, or a pair (num, den)),
        with mean_ap over 0.50 .. 0.95; match_of_a[a - 1] the label component a matched, or 0; ious the exact (a, b, num, den) of the
        matched pairs.  labels as in overlaps(): a ground truth, or components() of the previous frame."""
        return [capi.match_overlaps(rows, threshold) for rows in self.overlaps(labels, conn, invert, min_area, fill_holes, keep_largest, phase=phase)]

    def contours(self, conn=8, invert=False, min_area=0, fill_holes=0, keep_largest=False, simplify=None, subpixel=False, phase=0):
        """The boundary of every member's mask -- clean_masks' for the same options -- as ordered closed loops, traced on the device
        (cvh_contours_device_batch, ordered behind the current stream): one (loops, points) per member, loops a numpy structured array
        (capi.CONTOUR_LOOP_DTYPE), points an int32 device tensor (P, 2) of x, y, valid for the next operation on the current stream;
        bit for bit the member's own Context.contours().  Two sets of launches: the first for the counts that size the tensors.
        simplify (None: True) keeps the corners only.  subpixel=True (cvh_contours_subpixel_device_batch): the zero level of the level
        set instead -- one point per edge of the loops, where u changes sign across it; points a float64 device tensor (P, 2), bit for
        bit Context.contours_subpixel().  There is nothing to simplify then: simplify together with subpixel raises ValueError."""
        opts = dict(conn=conn, invert=invert, min_area=min_area, fill_holes=fill_holes, keep_largest=keep_largest)
        if subpixel:
            if simplify is not None:
                raise ValueError(f"contours: simplify = {simplify!r} together with subpixel=True (a subpixel loop has one point per edge)")
            batch, dtype = capi.contours_subpixel_batch, torch.float64
        else:
            batch, dtype = capi.contours_batch, torch.int32
            opts["simplify"] = True if simplify is None else simplify
        counts = batch(self._phase(phase), loop_caps=[0] * self.n, stream=self._stream(), **opts)
        points = [torch.empty((c[1], 2), dtype=dtype, device=torch.device("cuda", self.device)) for c in counts]
        rows = batch(self._phase(phase), [p.data_ptr() if p.numel() else 0 for p in points], [c[1] for c in counts],
                     loop_caps=[c[0] for c in counts], stream=self._stream(), **opts)
        return [(r[2], p) for r, p in zip(rows, points)]

    def levelsets(self, dtype=torch.float64, phase=0):
        """The members' level sets as a device tensor (N, H, W), float64 or float32 (rounded to nearest even)."""
        if dtype not in (torch.float64, torch.float32):
            raise ValueError(f"dtype must be float64 or float32, got {dtype}")
        out = torch.empty((self.n, self.h, self.w), dtype=dtype, device=torch.device("cuda", self.device))
        for i, ctx in enumerate(self._phase(phase)):
            ctx.get_levelset_device(out[i].data_ptr(), 64 if dtype == torch.float64 else 32, self._stream())
        return out

    def images(self):
        """The members' planes as they are now (after Perona-Malik: the smoothed image; with colour=: the converted planes of the last
        segment(), (Y, Cr, Cb) or (Y, U, V); with local= / rank=: the local / rank planes the run iterates on), (N, H, W) or (N, C, H, W) uint8."""
        shape = (self.n, self.h, self.w) if self.run_channels == 1 else (self.n, self.run_channels, self.h, self.w)
        out = torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", self.device))
        for i, ctx in enumerate(self.contexts):
            ctx.get_image_device(out[i].data_ptr(), capi.LAYOUT_PLANAR, self._stream())
        return out
