"""Connected components on the GPU (cvh_components*, cvh_get_mask_clean*) against the numpy restatement of the header's definition
(components_util).  Everything is defined in integers, so EVERY comparison is ==.  Run with -m gpu on an MI355X."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from chan_vese_amd import synth

import components_util as cu
import png_util
from test_gpu_device_io import Hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 144), (144, 1), (2, 2), (33, 257), (100, 517), (64, 2016), (512, 512)]
KINDS = ["rand50", "rand60", "spiral", "comb", "diagonal", "rings", "isolated", "inside", "outside", "special", "checkerboard", "after10"]
BIG = (1080, 1920)
ERR_ARG, ERR_STATE = 1, 3   # cvh_status
CLEAN_SETS = [(0, 0, 0), (5, 0, 0), (0, -1, 0), (0, 3, 0), (4, -1, 1), (0, 0, 1)]


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


@pytest.fixture()
def hip(capi):
    h = Hip()
    yield h
    h.free_all()


def noisy(h, w, channels=1, seed=5):
    return [synth.disk(max(h, w), 200 - 30 * k, 50 + 20 * k, noise=32, seed=seed + k, h=h, w=w) for k in range(channels)]


@functools.lru_cache(maxsize=None)
def levelset(kind, h, w):
    """the +-1 level sets of the issue (None: the context makes its own)"""
    rng = np.random.default_rng(h * 10007 + w)
    if kind in ("rand50", "rand60"):
        m = rng.random((h, w)) < (0.5 if kind == "rand50" else 0.6)
    elif kind in ("spiral", "comb", "diagonal", "rings", "isolated"):
        m = getattr(cu, kind)(h, w)
    elif kind == "inside":
        m = np.ones((h, w), bool)
    elif kind == "outside":
        m = np.zeros((h, w), bool)
    elif kind == "special":   # the sprinkling of test_gpu_reinit.py
        u = rng.standard_normal((h, w)) * 3
        flat = u.reshape(-1)
        for k, v in enumerate([np.nan, -0.0, 1e-60, -1e-60, 0.0, 1e-45, -np.nan, np.inf, -np.inf]):
            flat[(k * 7919 + 1) % flat.size::max(flat.size // 13, 1) + k] = v
        return u
    else:
        return None
    return np.where(m, 1.0, -1.0)


def give_levelset(ctx, kind, h, w):
    u = levelset(kind, h, w)
    if u is not None:
        ctx.set_levelset(u)
    else:
        ctx.init_checkerboard()
        if kind == "after10":
            ctx.run(10)


def make(capi, h, w, kind, channels=1, **opts):
    ctx = capi.Context(h, w, channels, capi.make_params(tol=0.0))
    ctx.set_option("co_resident", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.set_image(noisy(h, w, channels))
    give_levelset(ctx, kind, h, w)
    return ctx


def labels_of(ctx, hip, conn, invert, cap=None):
    d = hip.malloc(ctx.h * ctx.w * 4)
    k, table = ctx.components(conn, invert, labels_ptr=d, cap=cap)
    return hip.get(d, (ctx.h, ctx.w), np.int32), k, table


def check_labels(ctx, hip, conn, invert):
    want_l, want_t = cu.label(cu.foreground(ctx.get_levelset(), invert), conn)
    got_l, k, table = labels_of(ctx, hip, conn, invert)
    print(f"conn {conn} invert {invert}: K = {k} (restatement {want_t.size})")
    assert k == want_t.size
    assert np.array_equal(got_l, want_l)
    assert table.dtype == want_t.dtype and np.array_equal(table, want_t)
    return want_l, want_t


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labels_count_table(capi, hip, shape, kind):
    """1: labels, count and table are the restatement's, both connectivities, invert 0 and 1; cap < K; the NULL forms."""
    h, w = shape
    with make(capi, h, w, kind) as ctx:
        for conn in (4, 8):
            for invert in (False, True):
                want_l, want_t = check_labels(ctx, hip, conn, invert)
        K = want_t.size   # conn 8, inverted
        cap = K // 2
        got_l, k, table = labels_of(ctx, hip, 8, True, cap=cap)
        assert k == K and np.array_equal(got_l, want_l) and np.array_equal(table, want_t[:cap])
        k, table = ctx.components(8, True, labels_ptr=0, cap=K + 3)          # no label plane; more room than rows
        assert k == K and np.array_equal(table, want_t)
        k, table = ctx.components(8, True, labels_ptr=0, cap=0)              # neither
        assert k == K and table.size == 0


@pytest.mark.parametrize("kind,conn,invert", [("rand60", 4, False), ("comb", 8, False), ("checkerboard", 4, True)])
def test_labels_1080x1920(capi, hip, kind, conn, invert):
    h, w = BIG
    with make(capi, h, w, kind) as ctx:
        check_labels(ctx, hip, conn, invert)


def check_clean(capi, hip, shape, kind, forms=((4, False), (8, True))):
    h, w = shape
    with make(capi, h, w, kind) as ctx:
        u = ctx.get_levelset()
        d = hip.malloc(h * w + 3) + 3   # (any byte alignment)
        for conn, invert in forms:
            f = cu.foreground(u, invert)
            for min_area, fill, largest in CLEAN_SETS:
                want = cu.clean(f, conn, min_area, fill, bool(largest))
                got = ctx.get_mask_clean(conn, invert, min_area, fill, largest)
                ctx.get_mask_clean_device(d, conn, invert, min_area, fill, largest)
                dev = hip.get(d, (h, w), np.uint8)
                print(f"conn {conn} invert {invert} {(min_area, fill, largest)}: {int(want.sum())} set, {int((got != want).sum())} differ")
                assert np.array_equal(got, want)
                assert np.array_equal(dev, got)
                if (min_area, fill, largest) == (0, 0, 0):
                    assert np.array_equal(got, ctx.get_mask(invert))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_clean_mask(capi, hip, shape, kind):
    """2: the clean mask is the restatement's for the issue's six parameter sets, conn 4 plain and conn 8 inverted, on every shape and
    level set; host form == device form; (0, 0, 0) == get_mask.  (On 1 x N and N x 1 every pixel is on the border: no hole exists.)"""
    check_clean(capi, hip, shape, kind)


@pytest.mark.parametrize("conn,invert", [(4, False), (8, True)])
def test_clean_mask_1080x1920(capi, hip, conn, invert):
    """the six parameter sets on the level set of a noisy disk after 10 iterations (the restatement's time decides the case's)"""
    check_clean(capi, hip, BIG, "after10", ((conn, invert),))


def test_batch_forms(capi, hip):
    """3: five members of mixed shapes and channels, one uniform: each member == its own call; duplicate and NULL members are errors."""
    specs = [(100, 517, 1, "rand60"), (33, 257, 3, "after10"), (64, 2016, 1, "outside"), (2, 2, 1, "rand50"), (144, 1, 3, "special")]
    ctxs = [make(capi, h, w, kind, ch) for h, w, ch, kind in specs]
    try:
        for conn, invert in ((4, False), (8, True)):
            dl = [hip.malloc(c.h * c.w * 4) for c in ctxs]
            dl[3] = 0   # (a member without a label plane)
            counts = capi.components_batch(ctxs, dl, conn, invert)
            for i, c in enumerate(ctxs):
                want_l, k, _ = labels_of(c, hip, conn, invert, cap=0)
                assert counts[i] == k
                if dl[i]:
                    assert np.array_equal(hip.get(dl[i], (c.h, c.w), np.int32), want_l)
            assert capi.components_batch(ctxs, None, conn, invert) == counts
            dm = [hip.malloc(c.h * c.w) for c in ctxs]
            for params in ((4, -1, 1), (5, 0, 0), (0, 0, 0)):
                capi.get_mask_clean_device_batch(ctxs, dm, conn, invert, *params)
                for i, c in enumerate(ctxs):
                    assert np.array_equal(hip.get(dm[i], (c.h, c.w), np.uint8), c.get_mask_clean(conn, invert, *params))
        for call in (lambda m: capi.components_batch(m, None), lambda m: capi.get_mask_clean_device_batch(m, dm + dm[:1], min_area=3),
                     lambda m: capi.get_mask_clean_device_batch(m, dm + dm[:1])):   # (0, 0, 0): the route of the plain mask kernel
            with pytest.raises(capi.CvhError) as e:
                call(ctxs + ctxs[:1])
            assert e.value.code == ERR_ARG and "member 5 duplicates member 0" in str(e.value)
        L = capi.lib()
        arr = (capi.C.c_void_p * 2)(ctxs[0]._h, None)
        assert L.cvh_components_batch(arr, 2, 4, 0, None, None, None) == ERR_ARG
        assert b"member 1 is NULL" in L.cvh_last_error(None)
        with pytest.raises(capi.CvhError) as e:
            capi.components_batch(ctxs, None, conn=6)
        assert e.value.code == ERR_ARG
        with capi.Context(8, 8, 1, capi.make_params()) as empty:
            with pytest.raises(capi.CvhError) as e:
                capi.components_batch(ctxs + [empty], None)
            assert e.value.code == ERR_STATE and "member 5 has no level set" in str(e.value)
    finally:
        for c in ctxs:
            c.close()


def test_deterministic(capi, hip):
    """4a: the same call twice, and on a second context, gives identical bytes."""
    h, w = 100, 517
    outs = []
    for _ in range(2):
        with make(capi, h, w, "rand60") as ctx:
            for _ in range(2):
                l, k, t = labels_of(ctx, hip, 8, False)
                outs.append((l.tobytes(), k, t.tobytes(), ctx.get_mask_clean(8, False, 4, -1, True).tobytes()))
    assert all(o == outs[0] for o in outs[1:])


@pytest.mark.parametrize("opts", [{"resident": 0}, {"resident": 1}, {"state": 32}], ids=["per_launch", "resident", "state32"])
def test_no_side_effects(capi, hip, opts):
    """4b: 8 iterations, components + get_mask_clean, 8 more == 16 uninterrupted: level set, trace and steps."""
    h, w = 128, 256
    res = []
    for interrupt in (False, True):
        with make(capi, h, w, "checkerboard", **opts) as ctx:
            ctx.run(8)
            if interrupt:
                labels_of(ctx, hip, 4, False)
                ctx.get_mask_clean(8, False, 4, -1, True)
            steps, _ = ctx.run(8)
            res.append((steps, ctx.get_levelset().tobytes(), ctx.get_trace(32).tobytes()))
    assert res[0] == res[1]


def test_iterations_in_flight(capi, hip):
    """4c: with iterations enqueued and not synchronised the call equals sync followed by the call."""
    h, w = 100, 517
    res = []
    for sync_first in (False, True):
        with make(capi, h, w, "checkerboard") as ctx:
            ctx.enqueue_steps(6)
            if sync_first:
                ctx.sync()
            l, k, t = labels_of(ctx, hip, 4, False)
            res.append((l.tobytes(), k, t.tobytes(), ctx.get_mask_clean(4, False, 3, 2, False).tobytes()))
    assert res[0] == res[1]


def test_state32_class_from_float(capi, hip):
    """5: "state" = 32: a positive double below float's range is outside, as in cvh_reinit."""
    h, w = 33, 256   # ("state" = 32 takes widths that are multiples of 16)
    u = np.where(cu.rings(h, w), 1e-60, -1.0)
    u[5:9, 40:80] = 2.0
    with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_option("state", 32)
        ctx.set_image(noisy(h, w))
        ctx.set_levelset(u)
        want_l, want_t = cu.label(cu.foreground(u), 4)
        assert want_t.size == 1 and want_t["area"][0] == 160
        got_l, k, table = labels_of(ctx, hip, 4, False)
        assert k == 1 and np.array_equal(got_l, want_l) and np.array_equal(table, want_t)
        assert np.array_equal(ctx.get_mask_clean(4, False, 0, 0, True), cu.clean(cu.foreground(u), 4, 0, 0, True))


def test_argument_errors(capi, hip):
    """the rest of the header's CVH_ERR_ARG catalogue: parameters out of range, bad pointers; nothing is launched, the context stays usable"""
    h, w = 33, 257
    with make(capi, h, w, "rand60") as ctx:
        d = hip.malloc(h * w * 4 + 8)
        host = np.zeros((h, w), np.uint8)
        bad = [
            (lambda: ctx.get_mask_clean(4, False, -1, 0, 0), "min_area must not be negative"),
            (lambda: ctx.get_mask_clean(4, False, 0, -2, 0), "fill_holes must be -1"),
            (lambda: ctx.get_mask_clean(4, False, 0, 0, 2), "keep_largest must be 0 or 1"),
            (lambda: ctx.get_mask_clean(5, False, 0, 0, 0), "conn must be 4 or 8"),
            (lambda: ctx.get_mask_clean_device(d, 8, False, -3, 0, 0), "min_area must not be negative"),
            (lambda: ctx.get_mask_clean_device(0, 4, False, 3, 0, 0), "the device pointer is NULL"),
            (lambda: ctx.get_mask_clean_device(0, 4, False, 0, 0, 0), "the device pointer is NULL"),
            (lambda: ctx.get_mask_clean_device(host.ctypes.data, 4, False, 3, 0, 0), "is not device-accessible memory"),
            (lambda: ctx.get_mask_clean_device(host.ctypes.data, 4, False, 0, 0, 0), "is not device-accessible memory"),
            (lambda: ctx.components(4, False, labels_ptr=d + 2, cap=0), "is not aligned to 4 bytes"),
            (lambda: ctx.components(4, False, labels_ptr=host.ctypes.data, cap=0), "is not device-accessible memory"),
            (lambda: ctx.components(3, False, labels_ptr=d, cap=0), "conn must be 4 or 8"),
        ]
        for call, msg in bad:
            with pytest.raises(capi.CvhError) as e:
                call()
            assert e.value.code == ERR_ARG and msg in str(e.value), (msg, str(e.value))
        L, count = capi.lib(), capi.C.c_int(0)
        row = np.zeros(1, capi.COMPONENT_DTYPE)
        assert L.cvh_components(ctx._h, 4, 0, None, row.ctypes.data, -1, capi.C.byref(count), None) == ERR_ARG
        assert b"cap must not be negative" in L.cvh_last_error(ctx._h)
        assert L.cvh_get_mask_clean(ctx._h, None, 4, 0, 3, 0, 0) == ERR_ARG and b"mask is NULL" in L.cvh_last_error(ctx._h)
        check_labels(ctx, hip, 4, False)
    with capi.Context(8, 8, 1, capi.make_params()) as empty:
        for call in (lambda: empty.components(cap=0), lambda: empty.get_mask_clean(min_area=3), lambda: empty.get_mask_clean()):
            with pytest.raises(capi.CvhError) as e:
                call()
            assert e.value.code == ERR_STATE


def test_segmenter_on_a_caller_stream():
    """6: Segmenter.components and Segmenter.clean_masks on a side stream made current, in a child process (torch first: one HIP runtime)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_components_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch components child ok" in out.stdout


def test_cli(capi, tmp_path):
    """7: bin/chan_vese with the cleaning flags writes the restatement's _selection and --dump-mask and prints its --roi line; without
    them its files are those of cvh_separate and cvh_get_mask, as before, and stdout is empty."""
    h, w = 120, 176
    img = synth.disk(h, 190, 60, noise=48, seed=4, h=h, w=w)
    path = tmp_path / "in.png"
    path.write_bytes(png_util.encode(png_util.pack_samples(img, 8), w, h, 8, 0, [0, 1, 2]))
    cli = os.path.join(ROOT, "bin", "chan_vese")
    base = [cli, "-i", str(path), "-g", "-s", "-N", "12", "-t", "0", "--dump-mask", str(tmp_path / "m.pgm")]
    with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([img])
        ctx.init_checkerboard()
        assert ctx.run(12)[0] == 12
        u = ctx.get_levelset()
        img3 = np.repeat(img[:, :, None], 3, axis=2)
        plain_sel = {inv: ctx.separate(img3, inv) for inv in (False, True)}
        plain_mask = {inv: ctx.get_mask(inv) for inv in (False, True)}

    def outputs(r):
        assert r.returncode == 0, r.stderr
        sel = png_util.decode8((tmp_path / "in_selection.png").read_bytes()).reshape(h, w, 3)
        pgm = (tmp_path / "m.pgm").read_bytes()
        return sel, np.frombuffer(pgm[-h * w:], np.uint8).reshape(h, w)

    for inv in (False, True):
        r = subprocess.run(base + (["-I"] if inv else []), capture_output=True, text=True, timeout=600)
        sel, mask = outputs(r)
        assert r.stdout == "" and np.array_equal(sel, plain_sel[inv]) and np.array_equal(mask, plain_mask[inv] * 255)
    for inv, flags, (conn, min_area, fill, largest) in (
            (False, ["--min-area", "6", "--fill-holes", "-1", "--largest"], (4, 6, -1, True)),
            (True, ["--connectivity", "8", "--fill-holes", "3"], (8, 0, 3, False)),
            (False, ["--connectivity", "4"], (4, 0, 0, False))):
        r = subprocess.run(base + flags + ["--roi"] + (["-I"] if inv else []), capture_output=True, text=True, timeout=600)
        sel, mask = outputs(r)
        f = cu.foreground(u, inv)
        want = cu.clean(f, conn, min_area, fill, largest)
        assert np.array_equal(mask, want * 255)
        assert np.array_equal(sel, np.where(want[:, :, None] != 0, img3, 255))
        _, t = cu.label(cu.clean(f, conn, min_area, fill, True), conn)
        assert t.size == 1
        assert r.stdout == "roi %d %d %d %d %d\n" % (t["x0"][0], t["y0"][0], t["x1"][0], t["y1"][0], t["area"][0])
