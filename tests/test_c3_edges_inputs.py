"""The tables of tests/c3_edges_util.py, checked on the CPU: the inputs of tests/test_gpu_c3_edges.py are well-conditioned on the oracle at
every checkpoint (so its 1e-9 bars test the kernels), the shapes take the data flow and geometry they are named for, and the cases
between them name every instantiation of the two kernels."""
import numpy as np
import pytest

import c3_edges_util as K
import lopsided_util as L

INPUTS = ([(s, st, 3) for s in sorted(set(K.WAVE_SHAPES) | set(K.TILE_SHAPES)) for st in K.STARTS] +
          [(s, st, 1) for s in K.IMGV_THRESHOLD for st in K.STARTS])


@pytest.mark.parametrize("shape,start,channels", INPUTS, ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else str(v))
def test_oracle_is_conditioned_at_every_checkpoint(oracle, shape, start, channels):
    """A 1-ulp perturbation of u0 moves the oracle by <= 1e-11 of max|u| at 1, 2, 3 and 10 iterations (measured: <= 2e-12), and the run
    neither stops nor degenerates."""
    ref = K.reference(oracle, shape, start, channels)
    print("C3-COND %dx%d %s c%d %s" % (shape + (start, channels, {s: "%.1e" % v for s, v in ref["cond"].items()})))
    assert set(ref["cond"]) == set(K.CHECKPOINTS)
    assert max(ref["cond"].values()) <= K.COND_CAP, ref["cond"]
    for s in K.CHECKPOINTS:
        u, done, tr, m = ref["runs"][s]
        assert done == s and tr.shape == (s, 2 * channels + 1) and np.isfinite(u).all() and np.isfinite(tr).all()


def test_inputs_are_drawn_planes_first():
    h, w = 37, 53
    rng = np.random.default_rng(h * 7919 + w)
    planes = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)]
    u0 = rng.normal(size=(h, w))
    got_planes, got_u0, pk = K.inputs((h, w), "normal")
    assert all(np.array_equal(a, b) for a, b in zip(planes, got_planes)) and np.array_equal(u0, got_u0)
    assert pk == dict(tol=0, nu=0.01, lambda1=[1, 0.8, 0.5], lambda2=[0.7, 0.5, 1])
    one_planes, _, one_pk = K.inputs((h, w), "sdist", channels=1)
    assert len(one_planes) == 1 and np.array_equal(one_planes[0], planes[0]) and one_pk["lambda1"] == [1] and one_pk["lambda2"] == [0.7]
    _, sd, _ = K.inputs((4, 112), "sdist")
    assert sd[0, 0] == 4 / 3 - np.hypot(-2 + 0.3, -112 / 3 - 0.7)      # min(max(h, 3), max(w, 3)) / 3 - hypot(i - h/2 + 0.3, j - w/3 - 0.7)
    assert (sd > 0).any() and (sd < 0).any()


@pytest.mark.parametrize("mode", list(K.MODES))
def test_shapes_take_the_geometry_they_are_named_for(mode):
    """Host arithmetic of the library (cvh_debug_data_flow, no device): "kernel" = 2 is the 1-pixel wave kernel at every shape, with the
    wave columns the names promise; "kernel" = 3 falls back to it under STRICT; "kernel" = 0 is the tile kernel."""
    m = K.MODES[mode]
    for (h, w) in K.WAVE_SHAPES:
        kind, tx, ty, sr = L._data_flow(h, w, 3, m, 2, 64)
        assert kind == 2 and tx == (w + 62) // 63 and sr == 8 and ty == (h + 7) // 8, ((h, w), kind, tx, ty, sr)
    assert [(w + 62) // 63 for _, w in [(37, 53), (5, 63), (6, 64), (7, 127), (17, 1008), (3, 700)]] == [1, 1, 2, 3, 16, 12]
    for (h, w) in K.IMGV_THRESHOLD:
        assert L._data_flow(h, w, 1, m, 2, 64)[0] == 2 and K.is_imgv((h, w)) and not K.is_imgv((h, w), dict(wave_imgv=0))
    for (h, w) in [(33, 256), (17, 1008)]:
        assert L._data_flow(h, w, 3, m, 3, 64)[0] == (2 if mode == "strict" else 3)
    for (h, w) in K.TILE_SHAPES:
        kind, tx, ty, sr = L._data_flow(h, w, 3, m, 0, 64)
        assert kind == 0 and tx == (w + 255) // 256 and sr == 14 and ty == (h + 13) // 14, ((h, w), kind, tx, ty, sr)
    assert {s for s in K.WAVE_SHAPES if K.is_imgv(s)} == set(K.IMGV_THRESHOLD) | {(17, 1008), (33, 256)}
    assert not K.is_imgv((11, 88)) and not K.is_imgv((6, 64))


def test_option_sets_cover_modes_and_loaders():
    """Every option value meets STRICT and FAST (FAST-only options: FAST) on an IMGV shape and on a byte-load shape."""
    assert any(K.is_imgv(s) for s in K.OPTION_SHAPES) and any(not K.is_imgv(s) for s in K.OPTION_SHAPES)
    assert set(K.OPTION_SHAPES) <= set(K.WAVE_SHAPES)
    for name, (opts, modes) in K.WAVE_OPTIONS.items():
        fast_only = set(opts) & {"chain", "lut", "wave_pol"}
        assert set(modes) == ({"fast"} if fast_only else {"strict", "fast"}), name
    assert {tuple(o.items()) for o, _ in K.WAVE_OPTIONS.values()} >= {(("strip_rows", 8),), (("strip_rows", 5),), (("finalize", 1),),
                                                                      (("chain", 0),), (("lut", 0),), (("wave_pol", 1),)}
    assert any(h % 5 % 4 for h, _ in K.OPTION_SHAPES)      # strip_rows = 5: a strip that ends inside a 4-row group


def test_cases_name_every_instantiation():
    """What the cases of tests/test_gpu_c3_edges.py assert as launch_info()["kernel"], taken together."""
    wave = set()
    for shape in K.WAVE_SHAPES:
        wave.add(K.wave_name(3, "strict", shape))
    for name, (opts, modes) in K.WAVE_OPTIONS.items():
        for shape in K.OPTION_SHAPES:
            for mode in modes:
                wave.add(K.wave_name(3, mode, shape, opts, opts.get("wave_pol", 0)))
    want = {"csv_wave_kernel<3, false, false, 2, %s, 1, 0>" % i for i in ("true", "false")}
    want |= {"csv_wave_kernel<3, true, true, 3, %s, 1, %d>" % (i, p) for i in ("true", "false") for p in (0, 1)}
    want |= {"csv_wave_kernel<3, true, false, 3, %s, 1, 0>" % i for i in ("true", "false")}
    assert wave >= want, want - wave
    tile = {K.tile_name(r, m, l, s, d) for r, m, l in K.TILE_VARIANTS for s in K.TILE_SHAPES for d in (0, 1) if d == 0 or s[1] % 2 == 0}
    want = {"csv_step_kernel<3, %d, %s, %s>" % (r, fl, d) for r in (14, 16) for fl in ("false, false", "true, true", "true, false")
            for d in ("true", "false")}
    assert tile == want, tile ^ want
    assert K.wave_name(1, "strict", (3, 80)) == "csv_wave_kernel<1, false, false, 3, true, 1, 0>"
    assert K.wave_name(1, "fast", (3, 80), pol=1) == "csv_wave_kernel<1, true, true, 5, true, 1, 1>"
