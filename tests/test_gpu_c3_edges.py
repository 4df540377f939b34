"""Three channels in the two per-launch kernels a colour image takes by default -- csv_wave_kernel<3, ...> (every STRICT colour image,
FAST below 0.6 Mpixel, every width the 2-pixel kernel does not take) and csv_step_kernel<3, ...> (from 2^28 pixels) -- at the edges of
their geometry, against the oracle; and the aligned-piece image loader (IMGV) of the 1-pixel wave kernel at its threshold widths 80 .. 128
with one and three channels.  Shapes, option sets and inputs: tests/c3_edges_util.py.

Every case pins the instantiation through launch_info() before it runs, so it cannot silently run another kernel.

Bars (tests/test_gpu_parity.py), at 1, 2, 3 and 10 iterations, none skipped: level set within 1e-9 of max|u|, every trace row rtol 1e-9,
steps_done equal, the mask equal to the oracle's except where |u_cpu| <= 1e-9 max|u| (there, and only there, it may differ).  Every
case first asserts that the oracle itself moves by <= 1e-11 of max|u| (bar / 100) at each checkpoint under a 1-ulp perturbation of u0."""
import numpy as np
import pytest

import c3_edges_util as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from chan_vese_amd import capi as m
    m.lib()
    assert m.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return m


def sid(shape):
    return "%dx%d" % shape


def run_case(capi, oracle, shape, start, channels, mode, opts, expect):
    """One context, the four checkpoints.  expect(info) -> the kernel name this case must launch.  Returns the worst level-set error."""
    ref = K.reference(oracle, shape, start, channels)
    assert all(ref["cond"][s] <= K.COND_CAP for s in K.CHECKPOINTS), (shape, start, ref["cond"])
    h, w = shape
    worst = 0.0
    with capi.Context(h, w, channels, capi.make_params(**ref["pk"])) as ctx:
        ctx.set_option("math_mode", K.MODES[mode])
        for key, v in opts.items():
            ctx.set_option(key, v)
        ctx.set_option("trace", max(K.CHECKPOINTS))
        ctx.set_image(ref["planes"])
        for s in K.CHECKPOINTS:
            ctx.set_levelset(ref["u0"])
            info = ctx.launch_info()
            assert info["kernel"] == expect(info) and info["math"] == mode, (shape, mode, opts, info)
            done, _ = ctx.run(s)
            u_g, tr_g, m_g = ctx.get_levelset(), ctx.get_trace(s), ctx.get_mask()
            u_c, done_c, tr_c, m_c = ref["runs"][s]
            what = (sid(shape), start, channels, mode, opts, s)
            assert done == done_c == s, (what, done, done_c)
            scale = np.abs(u_c).max()
            err = float(np.abs(u_g - u_c).max() / scale)
            worst = max(worst, err)
            print("C3-EDGES %-24s %-9s %-6s c%d %-6s s=%-2d cond=%.1e err=%.2e %s" % (
                info["kernel"].split(",")[0] + ">", sid(shape), start, channels, mode, s, ref["cond"][s], err, opts))
            assert err <= K.BAR, (what, err)
            assert tr_g.shape == tr_c.shape and np.allclose(tr_g, tr_c, rtol=K.BAR, atol=0), (what, tr_g, tr_c)
            differs = m_g != m_c
            assert not (differs & (np.abs(u_c) > K.BAR * scale)).any(), (what, int(differs.sum()))
    return worst


def wave_expect(channels, mode, shape, opts):
    return lambda info: K.wave_name(channels, mode, shape, opts, int(info["wave_pol"]))


# ---- csv_wave_kernel<3, ...>

@pytest.mark.parametrize("mode", list(K.MODES))
@pytest.mark.parametrize("start", K.STARTS)
@pytest.mark.parametrize("shape", list(K.WAVE_SHAPES), ids=sid)
def test_wave_c3_shapes(capi, oracle, shape, start, mode):
    opts = dict(kernel=2)
    run_case(capi, oracle, shape, start, 3, mode, opts, wave_expect(3, mode, shape, opts))


WAVE_OPTION_CASES = [(name, shape, mode) for name, (_, modes) in K.WAVE_OPTIONS.items() for shape in K.OPTION_SHAPES for mode in modes]


@pytest.mark.parametrize("start", K.STARTS)
@pytest.mark.parametrize("name,shape,mode", WAVE_OPTION_CASES, ids=lambda v: sid(v) if isinstance(v, tuple) else v)
def test_wave_c3_options(capi, oracle, name, shape, mode, start):
    opts = dict(K.WAVE_OPTIONS[name][0], kernel=2)
    if "wave_pol" in opts:     # the store policy asked for is the one reported and the one instantiated
        expect = lambda info: K.wave_name(3, mode, shape, opts, opts["wave_pol"])
    else:
        expect = wave_expect(3, mode, shape, opts)
    run_case(capi, oracle, shape, start, 3, mode, opts, expect)


@pytest.mark.parametrize("mode", list(K.MODES))
@pytest.mark.parametrize("start", K.STARTS)
@pytest.mark.parametrize("channels", (3, 1))
@pytest.mark.parametrize("shape", K.IMGV_THRESHOLD, ids=sid)
def test_wave_byte_loads_at_the_imgv_widths(capi, oracle, shape, channels, start, mode):
    """"wave_imgv" = 0: the same bytes through the byte path (<..., false, 1, .>)."""
    opts = dict(kernel=2, wave_imgv=0)
    assert not K.is_imgv(shape, opts)
    run_case(capi, oracle, shape, start, channels, mode, opts, wave_expect(channels, mode, shape, opts))


@pytest.mark.parametrize("start", K.STARTS)
@pytest.mark.parametrize("shape", [(33, 256), (17, 1008)], ids=sid)
def test_two_pixel_request_falls_back_under_strict(capi, oracle, shape, start):
    """"kernel" = 3 with three channels in STRICT arithmetic: the 2-pixel kernel has no such flavour, the 1-pixel STRICT kernel runs."""
    opts = dict(kernel=3)
    expect = lambda info: K.wave_name(3, "strict", shape)
    assert expect(None).startswith("csv_wave_kernel<3, false, ")
    run_case(capi, oracle, shape, start, 3, "strict", opts, expect)


@pytest.mark.parametrize("mode", list(K.MODES))
@pytest.mark.parametrize("start", K.STARTS)
@pytest.mark.parametrize("shape", K.IMGV_THRESHOLD, ids=sid)
def test_wave_c1_at_the_imgv_widths(capi, oracle, shape, start, mode):
    """One channel: widths 80 .. 128 take IMGV only in this kernel (from 144 the 2-pixel kernel runs unless "kernel" = 2 is forced)."""
    opts = dict(kernel=2)
    expect = wave_expect(1, mode, shape, opts)
    assert K.is_imgv(shape) and ", true, 1, " in K.wave_name(1, mode, shape)
    run_case(capi, oracle, shape, start, 1, mode, opts, expect)


# ---- csv_step_kernel<3, ...>

@pytest.mark.parametrize("start", K.STARTS)
@pytest.mark.parametrize("rows,mode,lut", K.TILE_VARIANTS)
@pytest.mark.parametrize("shape", list(K.TILE_SHAPES), ids=sid)
def test_tile_c3(capi, oracle, shape, rows, mode, lut, start):
    name = K.tile_name(rows, mode, lut, shape, dma=0)
    run_case(capi, oracle, shape, start, 3, mode, K.tile_options(rows, mode, lut, dma=0), lambda info: name)


@pytest.mark.parametrize("start", K.STARTS)
@pytest.mark.parametrize("rows,mode,lut", K.TILE_VARIANTS)
@pytest.mark.parametrize("shape", [s for s in K.TILE_SHAPES if s[1] % 2 == 0], ids=sid)
def test_tile_c3_dma(capi, oracle, shape, rows, mode, lut, start):
    name = K.tile_name(rows, mode, lut, shape, dma=1)
    assert name.endswith(", true>")
    run_case(capi, oracle, shape, start, 3, mode, K.tile_options(rows, mode, lut, dma=1), lambda info: name)


@pytest.mark.parametrize("rows,mode,lut", K.TILE_VARIANTS)
@pytest.mark.parametrize("shape", [s for s in K.TILE_SHAPES if s[1] % 2 == 1], ids=sid)
def test_tile_c3_dma_falls_back_on_odd_widths(capi, shape, rows, mode, lut):
    """The LDS-DMA loader needs 16-byte aligned rows: on an odd width "dma" = 1 launches the register loader (csv_kernels.hip,
    launch_step_v) -- the very instantiation test_tile_c3 runs at this shape."""
    planes, u0, pk = K.inputs(shape, "normal")
    with capi.Context(shape[0], shape[1], 3, capi.make_params(**pk)) as ctx:
        ctx.set_option("math_mode", K.MODES[mode])
        for key, v in K.tile_options(rows, mode, lut, dma=1).items():
            ctx.set_option(key, v)
        ctx.set_image(planes)
        ctx.set_levelset(u0)
        info = ctx.launch_info()
    assert info["kernel"] == K.tile_name(rows, mode, lut, shape, dma=1) and info["kernel"].endswith(", false>"), info
