"""CPU side of the energy calls (include/chanvese_hip.h, "Energy"): the boundary -- header, exports, bindings, argument checking of the
Python drivers -- and the proposition the feature rests on, on the CPU oracle with the numpy restatement (energy_util.py): along a run
the functional falls."""
import ctypes
import os
import re

import numpy as np
import pytest

import energy_util as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def test_header_declares_and_library_exports(capi):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    assert "---- Energy ----" in hdr
    assert re.search(r"int cvh_energy\(cvh_context \*ctx, cvh_energy_terms \*out\);", hdr)
    assert re.search(r"int cvh_energy_batch\(cvh_context \*const \*ctxs, int n, cvh_energy_terms \*out\);", hdr)
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in ("cvh_energy", "cvh_energy_batch"):
        assert hasattr(raw, name) and name in capi.EXPORTS
    raw.cvh_debug_energy_launch_sets.restype = ctypes.c_ulong
    assert raw.cvh_debug_energy_launch_sets() >= 0


def test_struct_layout_matches_the_header(capi, tmp_path):
    """the ctypes struct and the C struct agree on size and on every offset"""
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text('#include "chanvese_hip.h"\n#include <stddef.h>\n#include <stdio.h>\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(cvh_energy_terms), offsetof(cvh_energy_terms, total),\n'
                   "  offsetof(cvh_energy_terms, length), offsetof(cvh_energy_terms, area), offsetof(cvh_energy_terms, fit_in),\n"
                   "  offsetof(cvh_energy_terms, fit_out), offsetof(cvh_energy_terms, c1), offsetof(cvh_energy_terms, c2)); return 0; }\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()]
    T = capi.EnergyTerms
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in ("total", "length", "area", "fit_in", "fit_out", "c1", "c2")]


def test_energy_without_gpu_fails_as_other_calls_do(capi):
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CvhError) as e:
        capi.Context(16, 16).energy()
    assert "no HIP device" in str(e.value)


def test_null_arguments_are_refused_without_a_device(capi):
    """what the library refuses before it touches a device: a NULL context, a NULL or empty list"""
    L = capi.lib()
    out = (capi.EnergyTerms * 1)()
    assert L.cvh_energy(None, out) != capi.CVH_OK
    for ctxs, n in ((None, 1), ((ctypes.c_void_p * 1)(None), 1), ((ctypes.c_void_p * 1)(None), 0)):
        assert L.cvh_energy_batch(ctxs, n, out) != capi.CVH_OK
        assert b"cvh_energy_batch" in L.cvh_last_error(None)
    with pytest.raises(capi.CvhError):
        capi.energy_batch([])


@pytest.mark.parametrize("kw", [dict(every=2.5), dict(every=True), dict(max_steps="10"), dict(max_steps=1.0), dict(rel_plateau=-1e-3),
                                dict(rel_plateau=float("nan")), dict(rel_plateau=float("inf")), dict(rel_plateau="x"),
                                dict(rel_plateau=True), dict(every=0, rel_plateau=1e-3), dict(every=-4, rel_plateau=0.0)])
def test_run_monitored_checks_its_arguments_first(capi, kw):
    """a ValueError before the context is touched: None stands in for it"""
    with pytest.raises(ValueError):
        capi.run_monitored(None, **kw)
    with pytest.raises(ValueError):
        capi.run_batch_monitored([None, None], **kw)


def test_monitored_drivers_on_a_stand_in(capi, monkeypatch):
    """the drivers' control flow without a device: contexts whose energy falls by a tenth per iteration until it freezes"""
    class Fake:
        channels = 1

        def __init__(self, freeze_at, stop_at):
            self.t, self.freeze_at, self.stop_at = 0, freeze_at, stop_at

        def run(self, k):
            done = max(0, min(k, self.stop_at - self.t))
            self.t += done
            return done, 1.0 / (1 + self.t)

        def sync(self):
            return self.t, 0.0, self.t >= self.stop_at

        def energy(self):
            return capi.Energy(100.0 * 0.9 ** min(self.t, self.freeze_at), 0.0, 0.0, (0.0,), (0.0,), (0.0,), (0.0,))

    monkeypatch.setattr(capi, "energy_batch", lambda cs: [c.energy() for c in cs])
    monkeypatch.setattr(capi, "run_batch", lambda cs, k: [c.run(k) for c in cs])
    steps, norm, series = capi.run_monitored(Fake(1000, 1000), max_steps=20, every=8)
    assert steps == 20 and [s for s, _ in series] == [8, 16, 20] and norm == 1.0 / 21
    steps, _, series = capi.run_monitored(Fake(12, 1000), every=8, rel_plateau=1e-6)
    assert [s for s, _ in series] == [8, 16, 24] and steps == 24   # the first segment that meets it: 16 -> 24 (frozen from 12 on), not later
    steps, _, series = capi.run_monitored(Fake(1000, 13), every=8, rel_plateau=1e-6)
    assert steps == 13 and [s for s, _ in series] == [8, 13]          # the stop rule fired inside the second segment
    steps, _, series = capi.run_monitored(Fake(1000, 1000), max_steps=30, every=0)
    assert steps == 30 and [s for s, _ in series] == [30]             # every <= 0: run(max_steps) plus one final energy
    res = capi.run_batch_monitored([Fake(4, 1000), Fake(1000, 10), Fake(1000, 1000)], max_steps=32, every=8, rel_plateau=1e-6)
    assert [r[0] for r in res] == [16, 10, 32]
    assert [[s for s, _ in r[2]] for r in res] == [[8, 16], [8, 10], [8, 16, 24, 32]]


# ---- the restatement's own facts ----
@pytest.mark.parametrize("h,w", E.SHAPES)
def test_restatement_facts(h, w):
    planes = E.planes_of("random", h, w, 3)
    for value in (0.0, 2.5, -7.0):
        assert E.terms(planes, np.full((h, w), value))["length"] == 0.0       # a constant u: every difference is an exact zero
    assert E.terms(planes, np.zeros((h, w)))["area"] == h * w / 2             # H(0) = 1/2 exactly
    # a constant image: c = I, every fit term 0.  All 0: exactly (0 / S = 0).  All 255: c = fl(fl(sum fl(255 H)) / fl(sum H)) -- four roundings,
    # |c - 255| <= 255 * 4 * 2^-53 to first order --, so a term is at most h w (255 * 2^-50)^2: 1e-31 of the 255^2 h w a term can reach
    t = E.terms(E.planes_of("all0", h, w, 3), E.smooth_levelset(h, w))
    assert t["fit_in"] == [0.0] * 3 and t["fit_out"] == [0.0] * 3
    t = E.terms(E.planes_of("all255", h, w, 3), E.smooth_levelset(h, w))
    assert max(t["fit_in"] + t["fit_out"]) <= h * w * (255 * 2.0 ** -50) ** 2, t


def test_restatement_nonfinite_terms():
    h, w = 17, 33
    planes = E.planes_of("random", h, w, 1)
    t = E.terms(planes, E.planted_levelset(h, w))
    assert not np.isfinite(E.flat(t)).any()                                   # a NaN reaches H, hence every sum and both means
    t = E.terms(planes, E.inf_levelset(h, w))
    assert np.isfinite([t["area"], *t["fit_in"], *t["fit_out"]]).all() and not np.isfinite(t["length"])   # H(+-inf) is 1 / 0; inf - u is not finite


# ---- the proposition, on the oracle ----
@pytest.mark.parametrize("n", [64, 128])
def test_energy_falls_along_an_oracle_run(oracle, n):
    _, series = E.oracle_series(n)
    assert [s for s, _ in series] == E.SAMPLES
    tot = [t["total"] for _, t in series]
    print(n, " ".join(f"{s}:{v:.6e}" for (s, _), v in zip(series, tot)), "length", series[0][1]["length"], "->", series[-1][1]["length"])
    assert all(b < a for a, b in zip(tot, tot[1:])), tot
    assert series[-1][1]["length"] < series[0][1]["length"]


def test_both_checkerboard_signs_end_alike(oracle):
    """default tolerance: the + and the - checkerboard stop at the same iteration with the same energy"""
    from chan_vese_amd import synth
    img = synth.disk(64, noise=32, seed=3)
    p = oracle.make_params()
    ends = []
    for sign in (1, -1):
        u, steps, _, _ = oracle.csv_run([img], sign * oracle.checkerboard(64, 64), p, 100000, trace=False)
        ends.append((steps, E.terms([img], u)["total"]))
    assert ends[0][0] == ends[1][0] and ends[0][0] < 100000, ends
    assert abs(ends[0][1] - ends[1][1]) <= 1e-12 * abs(ends[0][1]), ends
