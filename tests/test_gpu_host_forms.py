"""The single-context host forms that are batches of one member: cvh_init_checkerboard (a checkerboard batch of one), cvh_get_mask (the
batch mask kernel into the context's own buffer, then down) and the plane sums behind cvh_set_image (the ingest's adds on planes already on
the device).  Everything here is selections, integers or one IEEE product, so EVERY comparison is == (on bit patterns for level sets, traces
and means); nothing has a tolerance.  The shapes are the smallest at which these kernels can go wrong: no 16-pixel piece at all (1 x 1,
3 x 5), an n mod 16 tail (1 x 17, 40 x 33 x 3), a row longer than a workgroup (2 x 300), more rows than workgroups and more than one
workgroup per member (130 x 272), and widths that allow "state" = 32 (16 x 160, 130 x 272).  Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import init_util as U
from test_gpu_device_io import Hip

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 3
SHAPES = [(1, 1, 1), (1, 17, 1), (3, 5, 1), (2, 300, 1), (40, 33, 3), (16, 160, 1), (130, 272, 1)]
RUN_SHAPES = [(16, 160, 1), (130, 272, 1), (40, 33, 3)]
OPTIONS = {"default": {}, "per-launch": {"resident": 0}, "per-launch 1-pixel wave": {"resident": 0, "kernel": 2}}


def shape_id(s):
    return "x".join(str(v) for v in (s if s[2] == 3 else s[:2]))


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


def alone(ctx, **opts):
    """contexts compared in bits must not see each other in their automatic choices (tests/test_gpu_init.py)"""
    ctx.set_option("co_resident", 0)
    for k, v in opts.items():
        ctx.set_option(k, v)


def planes(h, w, channels):
    return U.planes_of("random", h, w, channels, seed=7)


def disk_start(h, w):
    i, j = np.mgrid[0:h, 0:w]
    return np.where((i - h / 2) ** 2 + (j - w / 2) ** 2 < (min(h, w) / 3 + 1) ** 2, 1.0, -1.0)


def edgy_levelset(h, w):
    """random doubles with the values the mask's float compare is about: both zeros, a positive double that rounds to 0.0f, NaN"""
    rng = np.random.default_rng(31 * h + w)
    u = rng.standard_normal((h, w))
    special = np.array([0.0, -0.0, 1e-60, -1e-60, np.nan, 1e-45, 3.0, -3.0])
    pick = rng.integers(0, 3 * special.size, (h, w))
    return np.where(pick < special.size, special[pick % special.size], u)


def iterate(ctx, k):
    ctx.enqueue_steps(k)
    done, nrm, _ = ctx.sync()
    return done, nrm, ctx.get_levelset(), ctx.get_trace(16), ctx.get_means()


def assert_same_run(a, b, k):
    assert a[0] == b[0] == k and a[1] == b[1]                                  # steps_done and the last norm
    assert np.array_equal(U.bits(a[2]), U.bits(b[2]))                           # level set
    assert a[3].shape == b[3].shape and a[3].shape[0] == k and np.array_equal(U.bits(a[3]), U.bits(b[3]))   # trace rows
    assert all(np.array_equal(U.bits(x), U.bits(y)) for x, y in zip(a[4], b[4]))                             # means


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_checkerboard_is_the_host_form_and_a_batch_of_one(capi, shape):
    h, w, channels = shape
    want = capi.checkerboard_host(h, w)
    with capi.Context(h, w, channels) as one, capi.Context(h, w, channels) as member:
        one.init_checkerboard()
        capi.init_checkerboard_batch([member])
        for ctx in (one, member):
            assert np.array_equal(U.bits(ctx.get_levelset()), U.bits(want))
            assert ctx.sync()[0] == 0


@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("shape", RUN_SHAPES, ids=shape_id)
def test_checkerboard_in_the_middle_of_a_run_is_set_levelset(capi, shape, options):
    """B iterates 3 times from another level set, then cvh_init_checkerboard, then 5 iterations; fresh A does cvh_set_levelset of the host
    checkerboard, then 5 iterations: level set, trace rows, means and steps_done agree bit for bit (B's chain-mode sum set is not set 0)"""
    h, w, channels = shape
    img = planes(h, w, channels)
    res = []
    for device in (True, False):
        with capi.Context(h, w, channels, capi.make_params(tol=0.0)) as ctx:
            alone(ctx, trace=16, **OPTIONS[options])
            ctx.set_image(img)
            if device:
                ctx.set_levelset(disk_start(h, w))
                assert iterate(ctx, 3)[0] == 3
                ctx.init_checkerboard()
            else:
                ctx.set_levelset(capi.checkerboard_host(h, w))
            assert ctx.sync()[0] == 0                                          # a new run
            start = ctx.get_levelset()
            res.append((start, iterate(ctx, 5)))
    assert np.array_equal(U.bits(res[0][0]), U.bits(res[1][0]))
    assert_same_run(res[0][1], res[1][1], 5)


def check_masks(ctx, hip, u):
    """every form of the plain mask against the definition on the level set u the context holds; twice (the reused device buffer and
    the pinned block's event)"""
    h, w = u.shape
    d_mask = hip.malloc(h * w)
    for invert in (0, 1):
        want = ((u.astype(np.float32) > 0) ^ bool(invert)).astype(np.uint8)
        got = ctx.get_mask(invert)
        assert got.dtype == np.uint8 and np.array_equal(got, want), invert
        ctx.get_mask_device(d_mask, invert)
        assert np.array_equal(hip.get(d_mask, (h, w), np.uint8), want), invert
        assert np.array_equal(ctx.get_mask_clean(4, invert, 0, 0, False), want), invert
        assert np.array_equal(ctx.get_mask(invert), got), invert


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_mask_is_the_definition_in_every_form(capi, hip, shape):
    h, w, channels = shape
    with capi.Context(h, w, channels) as ctx:
        ctx.set_levelset(edgy_levelset(h, w))
        u = ctx.get_levelset()
        assert np.array_equal(U.bits(u), U.bits(edgy_levelset(h, w)))
        check_masks(ctx, hip, u)


@pytest.mark.parametrize("shape", [(16, 160, 1), (130, 272, 1)], ids=shape_id)
def test_mask_of_an_fp32_state_with_a_stale_mirror(capi, hip, shape):
    h, w, channels = shape
    with capi.Context(h, w, channels, capi.make_params(tol=0.0)) as ctx:
        ctx.set_option("state", 32)
        ctx.set_image(planes(h, w, channels))
        ctx.init_checkerboard()
        ctx.enqueue_steps(3)
        assert ctx.sync()[0] == 3
        first = ctx.get_mask()                                                 # the double mirror is three iterations behind here
        u = ctx.get_levelset()
        assert np.array_equal(first, (u.astype(np.float32) > 0).astype(np.uint8))
        assert 0 < int(first.sum()) < h * w
        check_masks(ctx, hip, u)


def test_mask_settles_iterations_in_flight(capi):
    h, w = 130, 272
    with capi.Context(h, w, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image(planes(h, w, 1))
        ctx.init_checkerboard()
        ctx.enqueue_steps(3)                                                   # NOT synced: the getter has to settle them
        got = ctx.get_mask()
        assert ctx.sync()[0] == 3
        assert np.array_equal(got, (ctx.get_levelset().astype(np.float32) > 0).astype(np.uint8))


@pytest.mark.parametrize("shape", [(1, 17, 1), (3, 5, 1), (40, 33, 3)], ids=shape_id)
def test_plane_sums_of_set_image_are_the_ingest_s(capi, hip, shape):
    """the stop condition (tol = 1: the image norm) and the means after one iteration: cvh_set_image against cvh_set_image_device"""
    h, w, channels = shape
    img = planes(h, w, channels)
    res = []
    for device in (False, True):
        with capi.Context(h, w, channels, capi.make_params(tol=1.0)) as ctx:
            alone(ctx, resident=0)
            if device:
                ctx.set_image_device(hip.upload(np.stack(img)))
            else:
                ctx.set_image(img)
            assert all(np.array_equal(a, b) for a, b in zip(ctx.get_image(), img))
            ctx.init_checkerboard()
            stop = ctx.get_stop_condition()
            ctx.enqueue_steps(1)
            assert ctx.sync()[0] == 1
            res.append((stop, ctx.get_means()))
    assert res[0][0] == res[1][0]
    if channels == 1:                                                          # the exact integer sum of squares, one IEEE sqrt
        assert res[0][0] == np.sqrt(np.float64(int((img[0].astype(np.int64) ** 2).sum())))
    assert all(np.array_equal(U.bits(x), U.bits(y)) for x, y in zip(res[0][1], res[1][1]))


def test_error_forms_are_kept(capi):
    L = capi.lib()
    buf = np.zeros(15, dtype=np.uint8)
    assert L.cvh_get_mask(None, capi._u8p(buf), 0) == ERR_ARG
    assert L.cvh_init_checkerboard(None) == ERR_ARG
    with capi.Context(3, 5, 1) as ctx:
        assert L.cvh_get_mask(ctx._h, None, 0) == ERR_ARG
        with pytest.raises(capi.CvhError) as e:
            ctx.get_mask()
        assert e.value.code == ERR_STATE and "cvh_get_mask: no level set" in str(e.value)
        ctx.init_checkerboard()
        assert np.array_equal(ctx.get_mask(), (capi.checkerboard_host(3, 5) > 0).astype(np.uint8))
