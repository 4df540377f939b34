"""Parameter sets, initial level sets and images at the edges where the CSV kernels change path (tests/test_gpu_param_edges.py and the
oracle's own cross-check in tests/test_oracle_vs_numpy.py): eps far below and above 1 (almost no pixel / every pixel in the near field of
H_eps, whose far form starts at 32 eps), mu = 0 and large, both signs of nu, tiny and large dt, lambda1 != lambda2 with zeros; plateau,
outline, signed-distance and threshold-straddling starts; constant, all-zero, binary and single-pixel images."""
import numpy as np

from chan_vese_amd import synth

# A covering design rather than a product: every value of every parameter occurs in some set, and each GPU flavour runs every set.
# lambda1 / lambda2 are per channel (three-channel cases use all three entries, one-channel cases the first).
PARAMS = {
    "P0": dict(eps=0.05, mu=0.0, nu=-1.0, dt=0.01, lambda1=[0.0, 1.0, 4.0], lambda2=[4.0, 0.5, 1.0]),
    "P1": dict(eps=0.25, mu=2.5, nu=0.5, dt=3.0, lambda1=[4.0, 0.0, 1.0], lambda2=[0.0, 1.0, 0.5]),
    "P2": dict(eps=4.0, mu=2.5, nu=-1.0, dt=0.01, lambda1=[1.0, 4.0, 0.0], lambda2=[4.0, 0.0, 1.0]),
    "P3": dict(eps=16.0, mu=0.0, nu=0.5, dt=3.0, lambda1=[0.0, 0.5, 4.0], lambda2=[1.0, 4.0, 0.0]),
}
STARTS = ("checker", "rect", "circ", "sdist", "straddle")
IMAGES = ("disk", "const", "zero", "binary", "pixel")
PLATEAU = ("rect", "circ")   # flat regions: gradient 0/eta amplifies a 1-ulp difference ~1e6 per iteration (tests/test_golden.py)


def params(name, channels, **extra):
    p = dict(PARAMS[name])
    p["lambda1"], p["lambda2"] = p["lambda1"][:channels], p["lambda2"][:channels]
    p.update(extra)
    return p


def circle_outline(h, w, cx, cy, radius):
    """The CLI's --circ level set (chan_vese_amd/host/main.cpp draw_circle_outline): a 1-pixel midpoint-circle outline of ones on zeros."""
    u = np.zeros((h, w))

    def put(x, y):
        if 0 <= x < w and 0 <= y < h:
            u[y, x] = 1.0
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        for x, y in ((cx - dx, cy - dy), (cx + dx, cy - dy), (cx - dx, cy + dy), (cx + dx, cy + dy),
                     (cx - dy, cy - dx), (cx + dy, cy - dx), (cx - dy, cy + dx), (cx + dy, cy + dx)):
            put(x, y)
        dy += 1
        err += plus
        plus += 2
        mask = -1 if err > 0 else 0
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    return u


def start(oracle, kind, h, w, eps, seed=0):
    if kind == "checker":
        return oracle.checkerboard(h, w)
    if kind == "rect":
        return oracle.levelset_rect(h, w, w // 5, h // 4, w // 2, h // 2)
    if kind == "circ":
        return circle_outline(h, w, w // 2 - 3, h // 2 + 1, min(h, w) // 3)
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if kind == "sdist":       # signed distance to a circle: |u| up to the diagonal, in the far field from iteration 1
        return min(h, w) / 3 - np.hypot(ii - h / 2 + 0.3, jj - w / 3 - 0.7)
    if kind == "straddle":    # |u| within 10 % of 32 eps on both sides of the far threshold, signs of the checkerboard
        rng = np.random.default_rng(seed)
        return np.sign(oracle.checkerboard(h, w) - 0.5 + 1e-3) * 32.0 * eps * (1 + rng.uniform(-0.1, 0.1, size=(h, w)))
    raise ValueError(kind)


def image(kind, h, w, channels, seed=0):
    out = []
    for k in range(channels):
        if kind == "disk":
            p = synth.disk(min(h, w), 200 - 60 * k, 50 + 40 * k, noise=12, seed=seed + k, h=h, w=w)
        elif kind == "const":
            p = np.full((h, w), 117 + 20 * k, dtype=np.uint8)
        elif kind == "zero":
            p = np.zeros((h, w), dtype=np.uint8)
        elif kind == "binary":
            ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
            p = np.where(((ii // (3 + k)) + (jj // 5)) % 2 == 0, 255, 0).astype(np.uint8)
        elif kind == "pixel":
            p = np.zeros((h, w), dtype=np.uint8)
            p[h // 3 + k, (2 * w) // 3 - k] = 255
        else:
            raise ValueError(kind)
        out.append(np.ascontiguousarray(p, dtype=np.uint8))
    return out
