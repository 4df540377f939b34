"""The two definitions of include/chanvese_hip.h, "Edge-weighted length", restated in numpy op by op: the integer / IEEE Sobel edge map
(compared with `==`) and the edge-weighted iteration on np_restatement's heaviside / delta / normals (compared within 1e-9, the bar of
the four-phase kernels) -- with the cases and the demonstration scene.  Shared by test_geodesic_restatement.py (CPU) and the GPU tests."""
import functools
import math

import numpy as np

import init_util as I
import multiphase_util as M
import np_restatement as R

ONE = 32768
DEFAULT = M.DEFAULT
OTHER = M.OTHER_A
ITERATIONS = M.ITERATIONS
EDGE_K = 30.0

# ---- the edge map
EDGE_SHAPES = [(1, 7, 1), (7, 1, 1), (2, 2, 1), (3, 130, 1), (67, 65, 3), (8, 4096, 1)]
EDGE_KS = (0.5, 30.0, 1e6)


def sobel_m2(planes):
    """m2 = sum_k (sx_k^2 + sy_k^2), int64 (fits int32): the 3 x 3 Sobel sums of every plane with the coordinates clamped to the plane"""
    m2 = np.zeros(planes[0].shape, dtype=np.int64)
    for p in planes:
        f = np.pad(np.asarray(p).astype(np.int64), 1, mode="edge")
        sx = (f[:-2, 2:] + 2 * f[1:-1, 2:] + f[2:, 2:]) - (f[:-2, :-2] + 2 * f[1:-1, :-2] + f[2:, :-2])
        sy = (f[2:, :-2] + 2 * f[2:, 1:-1] + f[2:, 2:]) - (f[:-2, :-2] + 2 * f[:-2, 1:-1] + f[:-2, 2:])
        m2 += sx * sx + sy * sy
    return m2


def edge_den(C, K):
    return ((64.0 * C) * K) * K


def edge_map(planes, K):
    """gq = (uint16) rint(32768.0 / (1.0 + (double)m2 / den)): numpy's float64 division is IEEE, rint rounds half to even"""
    den = np.float64(edge_den(len(planes), float(K)))
    return np.rint(32768.0 / (1.0 + sobel_m2(planes).astype(np.float64) / den)).astype(np.uint16)


def checkers(h, w, channels=1):
    """0 / 255 checkers: the largest m2 a plane can have"""
    yy, xx = np.mgrid[0:h, 0:w]
    return [(((yy + xx + k) & 1) * 255).astype(np.uint8) for k in range(channels)]


def random_planes(h, w, channels, seed=5):
    rng = np.random.default_rng(seed + 31 * h + 7 * w + channels)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(channels)]


# ---- the iteration
def curvature_g(u, g):
    """kappa_g: np_restatement.curvature with Gx = g nx, Gy = g ny under the backward differences; the replicate pad gives the exact
    zeros of the border rule (Gx - Gx on column 0, Gy - Gy on row 0)"""
    eta2 = 1e-8 ** 2
    p = np.pad(u, 1, mode="edge")
    c = p[1:-1, 1:-1]
    upx = p[1:-1, 2:] - c
    upy = p[2:, 1:-1] - c
    ucx = 0.5 * (p[1:-1, 2:] - p[1:-1, :-2])
    ucy = 0.5 * (p[2:, 1:-1] - p[:-2, 1:-1])
    gx = g * (upx / np.sqrt(upx ** 2 + ucx ** 2 + eta2))
    gy = g * (upy / np.sqrt(upy ** 2 + ucy ** 2 + eta2))
    gxp = np.pad(gx, ((0, 0), (1, 0)), mode="edge")
    gyp = np.pad(gy, ((1, 0), (0, 0)), mode="edge")
    return (gx - gxp[:, :-1]) + (gy - gyp[:-1, :])


def weight(gq):
    return gq.astype(np.float64) * 2.0 ** -15


def means(planes, u, eps=1.0, backwards=False):
    """backwards: the same sums added in the reverse raster order -- another rounding of the same definition"""
    total = (lambda a: float(a.ravel()[::-1].sum())) if backwards else (lambda a: float(a.sum()))
    hv = R.heaviside(u, eps)
    c1 = [total(p.astype(np.float64) * hv) / total(hv) for p in planes]
    c2 = [total(p.astype(np.float64) * (1 - hv)) / total(1 - hv) for p in planes]
    return c1, c2


def step(planes, u, gq, p, backwards=False):
    """one iteration: (new u, c1, c2, ||d||)"""
    C = len(planes)
    with np.errstate(invalid="ignore", divide="ignore"):
        c1, c2 = means(planes, u, p["eps"], backwards)
    F = np.zeros_like(u)
    for k, img in enumerate(planes):
        f = img.astype(np.float64)
        F += -p["lambda1"][k] * (f - c1[k]) ** 2 + p["lambda2"][k] * (f - c2[k]) ** 2
    d = R.combine_folded(curvature_g(u, weight(gq)), F, p["mu"], p["nu"], p["dt"], C) * R.delta(u, p["eps"])
    return u + d, c1, c2, math.sqrt(float((d * d).sum()))


def run(planes, u, gq, p, max_steps, stop=None, backwards=False):
    """cvh_geodesic_run: (u, steps_done, trace) -- a trace row is [c1[0..C), c2[0..C), ||d||]"""
    if stop is None:
        stop = R.stop_condition(planes, p["tol"])
    rows = []
    for _ in range(max_steps):
        u, c1, c2, nrm = step(planes, u, gq, p, backwards)
        rows.append(list(c1) + list(c2) + [nrm])
        if nrm <= stop:
            break
    return u, len(rows), np.array(rows).reshape(len(rows), 2 * len(planes) + 1)


def mask(u):
    """cvh_get_mask(invert = 0): (float)u > 0"""
    return (u.astype(np.float32) > 0).astype(np.uint8)


# (h, w, channels, parameter set) of multiphase_util.CASES -- the wave-column seams and the strip seam -- each with a random edge plane
# and with the one the edge map gives for its image
CASES = [case + (kind,) for case in M.CASES for kind in ("random", "sobel")]


def case_id(case):
    h, w, C, which, kind = case
    return f"{h}x{w}x{C}-{which}-{kind}"


def params_of(which):
    return DEFAULT if which == "default" else OTHER


@functools.lru_cache(maxsize=None)
def case_inputs(h, w, C, kind):
    planes, u, _ = M.case_inputs(h, w, C)
    if kind == "random":
        gq = np.random.default_rng(17 + h + 3 * w).integers(0, ONE + 1, (h, w)).astype(np.uint16)
    elif kind == "ones":
        gq = np.full((h, w), ONE, dtype=np.uint16)
    else:
        gq = edge_map(planes, EDGE_K)
    gq.setflags(write=False)
    return planes, u, gq


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """the restatement's run of a case: computed once, shared, read-only"""
    h, w, C, which, kind = case
    planes, u, gq = case_inputs(h, w, C, kind)
    v, steps, trace = run(planes, u, gq, params_of(which), ITERATIONS)
    v.setflags(write=False)
    trace.setflags(write=False)
    return v, steps, trace


STOP_SHAPE = (24, 64, 1)


@functools.lru_cache(maxsize=None)
def stop_case():
    """(tol, k): with this tol the restatement stops at iteration k, 2 < k < 16 and k odd, with a factor of at least 1.05 between the
    stop condition and the norms on either side of it (random edge plane)"""
    planes, u, gq = case_inputs(*STOP_SHAPE, "random")
    _, _, trace = run(planes, u, gq, dict(DEFAULT, tol=0.0), 15)
    worst = trace[:, -1] / R.stop_condition(planes, 1.0)
    for k in range(3, 15, 2):
        before = worst[:k - 1].min()
        if worst[k - 1] * 1.05 ** 2 < before:
            tol = math.sqrt(worst[k - 1] * before)
            assert run(planes, u, gq, dict(DEFAULT, tol=tol), 40)[1] == k
            return tol, k
    raise AssertionError(f"no stopping iteration with a margin: {worst}")


# ---- the demonstration: a bright square with a thin arm on a dark ground, noisy; plain Chan-Vese against the edge-weighted length term
DEMO_MUS = (0.5, 5.0, 20.0, 100.0)
DEMO_KS = (5.0, 15.0, 45.0)
DEMO_PM = (30.0, 0.25, 2.0)   # K, L, T of the smoothing in front of the edge map
DEMO_STEPS = 300


@functools.lru_cache(maxsize=None)
def demo_scene():
    """(noisy uint8 plane, clean bool shape, the arm's bool pixels): 64 x 64, square 16..40 x 12..36, a 3 px arm to the right, sigma 20"""
    shape = np.zeros((64, 64), dtype=bool)
    shape[16:40, 12:36] = True
    arm = np.zeros_like(shape)
    arm[26:29, 36:56] = True
    shape |= arm
    rng = np.random.default_rng(2024)
    img = np.where(shape, 170.0, 70.0) + rng.normal(0.0, 20.0, shape.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), shape, arm


def demo_start(img):
    """Otsu start as cvh_init_otsu(inside = 1, outside = -1)"""
    t = I.otsu(I.histogram([img]))
    return I.start_threshold([img], t, 1.0, -1.0), t


def demo_smoothed(img):
    K, L, T = DEMO_PM
    trips = int(math.ceil(T / L - 1e-9))
    return R.perona_malik(img, K, L, trips)[0]


def components(m):
    """4-connected components of a bool mask (count), by flood fill: 64 x 64 only"""
    seen = np.zeros_like(m, dtype=bool)
    count = 0
    for r, c in zip(*np.nonzero(m)):
        if seen[r, c]:
            continue
        count += 1
        stack = [(r, c)]
        seen[r, c] = True
        while stack:
            y, x = stack.pop()
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < m.shape[0] and 0 <= xx < m.shape[1] and m[yy, xx] and not seen[yy, xx]:
                    seen[yy, xx] = True
                    stack.append((yy, xx))
    return count


def demo_score(m, shape, arm):
    """(IoU with the clean shape, speckle = components of mask and of its complement beyond one each, share of the arm kept)"""
    m = m.astype(bool)
    iou = (m & shape).sum() / (m | shape).sum()
    speckle = max(components(m) - 1, 0) + max(components(~m) - 1, 0)
    return float(iou), int(speckle), float((m & arm).sum() / arm.sum())


def demo_params(mu):
    """lambda = 1e-3: the data term of an 8-bit image (squared grey differences, up to 10^4 here) brought to the order of mu kappa.
    With lambda = 1 and dt = 1 the first iteration moves every pixel hundreds of eps away from the front, delta_eps vanishes, and the mask
    stays the first iteration's threshold at every mu tried: neither length term has anything to say."""
    return dict(DEFAULT, mu=mu, dt=demo_dt(mu), tol=0.0, lambda1=(1e-3,) * 3, lambda2=(1e-3,) * 3)


DEMO_DT_MU = 5.0   # the explicit scheme's step: dt mu <= 5


def demo_dt(mu):
    """dt = 1 up to mu = 5, then 5 / mu.  With dt = 1 at mu = 20 and 100 the explicit curvature step is unstable and the run chaotic: the
    restatement ITSELF, with nothing changed but the order in which the means' sums are added, ends with 11 / 54 / 29 other pixels in its
    mask (plain mu = 20, plain mu = 100, weighted mu = 100 K = 45) and level sets up to 100 apart -- there is no "the restatement's mask"
    to hold a device to.  With dt mu <= 5 the same experiment flips no pixel in any run (test_geodesic_restatement.py)."""
    return min(1.0, DEMO_DT_MU / mu)


def demo_steps(mu):
    """the same evolution time at every mu: DEMO_STEPS / dt iterations"""
    return int(round(DEMO_STEPS / demo_dt(mu)))


@functools.lru_cache(maxsize=None)
def demo_runs():
    """({name: (mask, iou, speckle, arm, firm)}, best mu) of the plain runs at DEMO_MUS and of the weighted runs at the smallest
    speckle-free mu and above.  firm: the pixels on which the restatement itself is determinate -- the run repeated with the means' sums
    added in the reverse order gives the same mask there, and both level sets lie further from the front than they lie from each other.
    It is the restatement's own error, taken without any device; a device's mask is held to the restatement's on the firm pixels."""
    img, shape, arm = demo_scene()
    u0, _ = demo_start(img)
    ones = np.full(img.shape, ONE, dtype=np.uint16)
    out = {}

    def one(name, gq, mu):
        a = run([img], u0, gq, demo_params(mu), demo_steps(mu))[0]
        b = run([img], u0, gq, demo_params(mu), demo_steps(mu), backwards=True)[0]
        firm = (mask(a) == mask(b)) & (np.minimum(np.abs(a), np.abs(b)) > np.abs(a - b))
        out[name] = (mask(a),) + demo_score(mask(a), shape, arm) + (firm,)

    for mu in DEMO_MUS:
        one(f"plain mu={mu:g}", ones, mu)
    clean = [mu for mu in DEMO_MUS[1:] if out[f"plain mu={mu:g}"][2] == 0]
    best = clean[0] if clean else DEMO_MUS[-1]
    smooth = demo_smoothed(img)
    for mu in [mu for mu in DEMO_MUS if mu >= best]:   # (at that mu, and at the larger ones: what over-smoothing costs either model)
        for K in DEMO_KS:
            one(f"edge mu={mu:g} K={K:g}", edge_map([smooth], K), mu)
    return out, best
