"""The primal-dual iteration of include/chanvese_hip.h, "Convex relaxation", restated in numpy operation by operation -- what the
device is compared against (test_gpu_convex.py, test_gpu_convex_batch.py) and what the CPU tests state facts about
(test_convex_restatement.py) -- with a second restatement in plain loops, the parameter sets, the cases and the disk scene.

Every array operation below is one IEEE operation per element, in the contract's order: numpy neither fuses nor reorders them, so with
means_every = 0 (the means come from exact integer sums) every value of a run is bit-defined.  The sums behind retaken means and the
norm are numpy's pairwise sums; the device adds in another fixed order, which is what the 1e-9 of the GPU tests covers."""
import functools
import math

import numpy as np

import multiphase_util as M

ITERATIONS = 6
ONE = 32768
# set A is the issue's; set B: unequal lambdas, nu != 0, the larger primal step, means retaken every iteration
SET_A = dict(mu=0.5, nu=0.0, lambda1=(1e-4, 1e-4, 1e-4), lambda2=(1e-4, 1e-4, 1e-4), tau=0.25, sigma=0.5, means_every=2)
SET_B = dict(mu=0.3, nu=0.02, lambda1=(1.2e-4, 0.9e-4, 1.1e-4), lambda2=(0.8e-4, 1.1e-4, 1.0e-4), tau=0.5, sigma=0.25, means_every=1)
SETS = {"A": SET_A, "B": SET_B}
SHAPES = sorted({c[:3] for c in M.CASES}, key=lambda s: (s[0] * s[1], s))


def shape_id(shape):
    return "x".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def case_inputs(h, w, C):
    """(planes, level set, random edge plane): multiphase_util's planes and its checkerboard start"""
    planes, u, _ = M.case_inputs(h, w, C)
    gq = np.random.default_rng(1000 * h + w).integers(0, ONE + 1, (h, w)).astype(np.uint16)
    gq.setflags(write=False)
    return planes, u, gq


def mask(u):
    """cvh_get_mask with invert = 0"""
    return (np.asarray(u, dtype=np.float64).astype(np.float32) > 0).astype(np.uint8)


def means(planes, v):
    """c1[k] = sum f v / sum v, c2[k] = (sum f - sum f v) / (h w - sum v): the complement, no guard"""
    sv = float(np.sum(v))
    c1, c2 = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for img in planes:
            f = img.astype(np.float64)
            sfv = float(np.sum(f * v))
            c1.append(np.float64(sfv) / np.float64(sv))
            c2.append((np.float64(float(np.sum(img, dtype=np.int64))) - np.float64(sfv)) / (np.float64(float(v.size)) - np.float64(sv)))
    return [float(x) for x in c1], [float(x) for x in c2]


def start(planes, u):
    v = mask(u).astype(np.float64)
    c1, c2 = means(planes, v)
    return dict(v=v, vbar=v.copy(), qx=np.zeros_like(v), qy=np.zeros_like(v), c1=c1, c2=c2, since=0)


def step(planes, st, p, gq, stats=None):
    """one Jacobi iteration of the contract from state st: (v', vbar', qx', qy', ||d||); stats, if given, counts the branches"""
    C = len(planes)
    v, vbar, qx, qy = st["v"], st["vbar"], st["qx"], st["qy"]
    tau, sigma, mu, nu = p["tau"], p["sigma"], p["mu"], p["nu"]
    t = []
    for k, img in enumerate(planes):
        f = img.astype(np.float64)
        a, b = f - st["c1"][k], f - st["c2"][k]
        t.append(p["lambda1"][k] * (a * a) - p["lambda2"][k] * (b * b))
    r = nu + t[0] if C == 1 else nu + ((t[0] + t[1]) + t[2]) / float(C)
    dx = np.pad(vbar[:, 1:] - vbar[:, :-1], ((0, 0), (0, 1)))
    dy = np.pad(vbar[1:] - vbar[:-1], ((0, 1), (0, 0)))
    tx, ty = qx + sigma * dx, qy + sigma * dy
    s = np.sqrt(tx * tx + ty * ty)
    rho = mu * (gq.astype(np.float64) * 2.0 ** -15) if gq is not None else np.full_like(v, mu * 1.0)
    take = s > rho
    with np.errstate(divide="ignore", invalid="ignore"):
        k = rho / s
        nqx, nqy = np.where(take, tx * k, tx), np.where(take, ty * k, ty)
    div = (nqx - np.pad(nqx[:, :-1], ((0, 0), (1, 0)))) + (nqy - np.pad(nqy[:-1], ((1, 0), (0, 0))))
    x = v + tau * (div - r)
    nv = np.where(x < 0, 0.0, np.where(x > 1, 1.0, x))
    nvbar = (nv + nv) - v
    d = nv - v
    if stats is not None:
        stats["pixels"] = stats.get("pixels", 0) + v.size
        for name, m in (("taken", take), ("not_taken", ~take), ("clamp0", x < 0), ("clamp1", x > 1), ("no_clamp", (x >= 0) & (x <= 1))):
            stats[name] = stats.get(name, 0) + int(m.sum())
    return nv, nvbar, nqx, nqy, math.sqrt(float(np.sum(d * d)))


def run(planes, u, gq, p, max_steps, stop_rms=-1.0, means_every=None, state=None, stats=None):
    """cvh_convex_run: (state, steps_done, trace); state = None starts from the mask of u, else resumes (u is not read)"""
    st = dict(state) if state is not None else start(planes, u)
    every = p["means_every"] if means_every is None else means_every
    stop = stop_rms * math.sqrt(float(st["v"].size))
    rows = []
    for _ in range(max_steps):
        nv, nvbar, nqx, nqy, nrm = step(planes, st, p, gq, stats)
        rows.append(list(st["c1"]) + list(st["c2"]) + [nrm])
        st.update(v=nv, vbar=nvbar, qx=nqx, qy=nqy, since=st["since"] + 1)
        if every > 0 and st["since"] >= every:
            st["c1"], st["c2"] = means(planes, nv)
            st["since"] = 0
        if stop_rms >= 0 and nrm <= stop:
            break
    return st, len(rows), np.array(rows, dtype=np.float64).reshape(len(rows), 2 * len(planes) + 1)


def step_loops(planes, st, p, gq):
    """the same iteration pixel by pixel on Python floats (IEEE doubles, one rounding per operation): (v', vbar', qx', qy')"""
    C = len(planes)
    h, w = st["v"].shape
    v, vbar, qx, qy = (st[n].tolist() for n in ("v", "vbar", "qx", "qy"))
    tau, sigma, mu, nu = p["tau"], p["sigma"], p["mu"], p["nu"]
    nqx, nqy = [[0.0] * w for _ in range(h)], [[0.0] * w for _ in range(h)]
    for r in range(h):
        for c in range(w):
            dx = vbar[r][c + 1] - vbar[r][c] if c < w - 1 else 0.0
            dy = vbar[r + 1][c] - vbar[r][c] if r < h - 1 else 0.0
            tx, ty = qx[r][c] + sigma * dx, qy[r][c] + sigma * dy
            s = math.sqrt(tx * tx + ty * ty)
            rho = mu * (float(gq[r, c]) * 2.0 ** -15 if gq is not None else 1.0)
            if s > rho:
                k = rho / s
                nqx[r][c], nqy[r][c] = tx * k, ty * k
            else:
                nqx[r][c], nqy[r][c] = tx, ty
    nv, nvbar = [[0.0] * w for _ in range(h)], [[0.0] * w for _ in range(h)]
    for r in range(h):
        for c in range(w):
            t = []
            for k in range(C):
                f = float(planes[k][r, c])
                a, b = f - st["c1"][k], f - st["c2"][k]
                t.append(p["lambda1"][k] * (a * a) - p["lambda2"][k] * (b * b))
            rr = nu + t[0] if C == 1 else nu + ((t[0] + t[1]) + t[2]) / float(C)
            div = (nqx[r][c] - (nqx[r][c - 1] if c > 0 else 0.0)) + (nqy[r][c] - (nqy[r - 1][c] if r > 0 else 0.0))
            x = v[r][c] + tau * (div - rr)
            nv[r][c] = 0.0 if x < 0 else (1.0 if x > 1 else x)
            nvbar[r][c] = (nv[r][c] + nv[r][c]) - v[r][c]
    return tuple(np.array(a, dtype=np.float64) for a in (nv, nvbar, nqx, nqy))


def gradient(v):
    """the forward differences of the contract: zero behind the last column / row"""
    return np.pad(v[:, 1:] - v[:, :-1], ((0, 0), (0, 1))), np.pad(v[1:] - v[:-1], ((0, 1), (0, 0)))


def divergence(qx, qy):
    """the backward differences of the contract: the value itself on the first column / row"""
    return (qx - np.pad(qx[:, :-1], ((0, 0), (1, 0)))) + (qy - np.pad(qy[:-1], ((1, 0), (0, 0))))


@functools.lru_cache(maxsize=None)
def reference(shape, which, use_edge, means_every=None, steps=ITERATIONS):
    """the restatement's run of a case: (v, qx, qy, steps_done, trace), computed once, shared, read-only"""
    planes, u, gq = case_inputs(*shape)
    st, done, trace = run(planes, u, gq if use_edge else None, SETS[which], steps, means_every=means_every)
    out = (st["v"], st["qx"], st["qy"], trace)
    for a in out:
        a.setflags(write=False)
    return out[0], out[1], out[2], done, out[3]


@functools.lru_cache(maxsize=None)
def branch_shares(shape, which, use_edge):
    """{branch: share of the pixel-iterations of the case's 6 iterations}, and the share of pixels with 0 < v < 1 at the end"""
    planes, u, gq = case_inputs(*shape)
    stats = {}
    st, _, _ = run(planes, u, gq if use_edge else None, SETS[which], ITERATIONS, stats=stats)
    v = st["v"]
    shares = {k: n / stats["pixels"] for k, n in stats.items() if k != "pixels"}
    return shares, float(((v > 0) & (v < 1)).mean())


# ---- the disk scene of the issue: a noisy disk from the mask of the checkerboard, lambda = 1e-3, means retaken every iteration
DISK = dict(mu=0.5, nu=0.0, lambda1=(1e-3,) * 3, lambda2=(1e-3,) * 3, tau=0.25, sigma=0.5, means_every=1)


@functools.lru_cache(maxsize=None)
def disk_scene(n=64):
    """(plane, truth): chan_vese_amd.synth.disk(n, noise=32, seed=3), the README's noisy disk, and the disk itself"""
    from chan_vese_amd import synth
    img = synth.disk(n, noise=32, seed=3)
    img.setflags(write=False)
    return img, synth.disk(n) > 100


@functools.lru_cache(maxsize=None)
def disk_reference(n=64):
    """the restatement's run of the disk scene to an exact fixed point: (v, steps_done, trace)"""
    img, _ = disk_scene(n)
    u = M.starts(n, n)[0]
    st, done, trace = run([img], u, None, DISK, 64, stop_rms=0.0)
    return st["v"], done, trace


# ---- the demonstration: the relaxation against the level-set descent (geodesic_util's restatement; an edge plane of ones is the
# two-phase model) on three scenes.  Rows are computed on the restatements once; tools/convex_probe.py --demo repeats them on the card.
DEMO_STOP = 1e-5      # stop_rms of the convex runs
DEMO_BUDGET = 3000    # their bound
DEMO_LS_STEPS = 300   # the level-set runs: tol = 0 (the grey-level stop rule fires at once where lambda is scaled down), this many iterations


@functools.lru_cache(maxsize=None)
def hard_scene(n=64, seed=7):
    """(b) (plane, truth): a disk of grey level 150 on 100 with Gaussian noise of sigma 40 -- the noise is the contrast's size, a
    threshold cannot segment it (IoU about 1/3), the length term has to"""
    yy, xx = np.mgrid[0:n, 0:n]
    truth = (xx - (n - 1) / 2.0) ** 2 + (yy - (n - 1) / 2.0) ** 2 <= (n / 4.0) ** 2
    g = np.where(truth, 150.0, 100.0) + np.random.default_rng(seed).normal(0.0, 40.0, (n, n))
    img = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    img.setflags(write=False)
    return img, truth


def convex_set(mu, lam, tau=0.25, sigma=0.5):
    return dict(mu=mu, nu=0.0, lambda1=(lam,) * 3, lambda2=(lam,) * 3, tau=tau, sigma=sigma, means_every=1)


def demo_cases():
    """[(scene, run name, plane, truth, start, edge plane or None, convex set or None, level-set parameters or None)]"""
    import geodesic_util as G
    out = []
    img, truth = disk_scene()
    cb = M.starts(64, 64)[0]
    out.append(("a-disk", "convex mu=0.5 lambda=1e-3", img, truth, cb, None, DISK, None))
    out.append(("a-disk", "level set mu=0.5 lambda=1", img, truth, cb, None, None, dict(G.DEFAULT, tol=0.0)))
    img, truth = hard_scene()
    for mu in (0.0, 0.2, 0.5, 1.0):   # lambda = 1e-4: tau |r| is about 0.1 (demo_rows reports it)
        out.append(("b-hard", f"convex mu={mu:g} lambda=1e-4", img, truth, cb, None, convex_set(mu, 1e-4), None))
    for mu, lam in ((0.5, 1e-4), (5.0, 1e-3), (0.5, 1.0)):
        out.append(("b-hard", f"level set mu={mu:g} lambda={lam:g}", img, truth, cb, None, None,
                    dict(G.DEFAULT, mu=mu, tol=0.0, lambda1=(lam,) * 3, lambda2=(lam,) * 3)))
    img, shape, _ = G.demo_scene()
    u0, _ = G.demo_start(img)
    smooth = G.demo_smoothed(img)
    for mu in (0.5, 5.0):
        out.append(("c-arm", f"convex mu={mu:g} lambda=1e-3", img, shape, u0, None, convex_set(mu, 1e-3), None))
        for K in G.DEMO_KS:
            out.append(("c-arm", f"convex edge K={K:g} mu={mu:g} lambda=1e-3", img, shape, u0, G.edge_map([smooth], K), convex_set(mu, 1e-3), None))
    out.append(("c-arm", "level set mu=5 lambda=1e-3", img, shape, u0, None, None, G.demo_params(5.0)))
    out.append(("c-arm", "level set edge K=15 mu=5 lambda=1e-3", img, shape, u0, G.edge_map([smooth], 15.0), None, G.demo_params(5.0)))
    return out


@functools.lru_cache(maxsize=None)
def demo_rows():
    """one dict per run of demo_cases() on the restatements: iterations (convex: to the stop rule), IoU with the clean shape, speckle
    (components of the mask and of its complement beyond one each), and for a convex run the share of 0 < v < 1, the IoU of the plain
    threshold at (c1 + c2) / 2 -- what the run would be without its length term -- and the mean of tau |r|; `mask` is the run's mask"""
    import geodesic_util as G
    rows = []
    for scene, name, img, truth, u0, gq, cset, lset in demo_cases():
        row = dict(scene=scene, run=name)
        if cset is not None:
            st, done, _ = run([img], u0, gq, cset, DEMO_BUDGET, stop_rms=0.0 if scene == "a-disk" else DEMO_STOP)
            m = st["v"] > 0.5
            f = img.astype(np.float64)
            r = cset["lambda1"][0] * (f - st["c1"][0]) ** 2 - cset["lambda2"][0] * (f - st["c2"][0]) ** 2
            thr = f > (st["c1"][0] + st["c2"][0]) / 2
            row.update(iterations=done, stopped=done < DEMO_BUDGET, between=round(float(((st["v"] > 0) & (st["v"] < 1)).mean()), 4),
                       threshold_iou=round(float((thr & truth).sum() / (thr | truth).sum()), 4), tau_r=round(float(cset["tau"] * np.abs(r).mean()), 3))
        else:
            ones = np.full(img.shape, ONE, dtype=np.uint16)
            u, done, _ = G.run([img], u0, ones if gq is None else gq, lset, DEMO_LS_STEPS)
            m = G.mask(u).astype(bool)
            row.update(iterations=done, stopped=False)
        iou, speckle, _ = G.demo_score(m, truth, truth)
        row.update(iou=round(iou, 4), speckle=speckle, mask=m)
        rows.append(row)
    return rows
