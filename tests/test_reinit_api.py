"""Level-set reinitialisation without a GPU: the numpy checker (reinit_util.signed_edt) against an all-pairs minimum, the exported
symbols, the argument errors a batch call can decide before it touches a device, the helpers' delegation and the CLI's validation."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import reinit_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


def structured_masks():
    out = {}
    m = np.zeros((9, 11), bool); m[4, 5] = True
    out["single pixel"] = m
    out["single hole"] = ~m
    m = np.zeros((12, 24), bool); m[:, ::3] = True
    out["column stripes"] = m
    m = np.zeros((24, 12), bool); m[::5] = True
    out["row stripes"] = m
    m = np.zeros((24, 24), bool); m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    out["corners"] = m
    out["one outside corner"] = ~np.pad(np.ones((1, 1), bool), ((0, 23), (0, 23)))
    m = np.zeros((1, 23), bool); m[0, 3:7] = True; m[0, 20] = True
    out["1 x N"] = m
    out["N x 1"] = m.T.copy()
    m = np.zeros((2, 2), bool); m[0, 0] = True
    out["2 x 2"] = m
    return out


@pytest.mark.parametrize("name", sorted(structured_masks()))
@pytest.mark.parametrize("window", [64, 2])
def test_signed_edt_structured(name, window):
    m = structured_masks()[name]
    u = np.where(m, 3.0, -2.0)
    d2, un, changed = R.signed_edt(u, window=window)
    assert changed
    ref = R.naive_d2(m)
    assert np.array_equal(d2, ref)
    assert np.array_equal(R.bits(un), R.bits(np.where(m, 1.0, -1.0) * (np.sqrt(ref.astype(np.float64)) - 0.5)))
    assert np.array_equal(R.mask_of(un), m) and np.abs(un).min() >= 0.5


@pytest.mark.parametrize("seed", range(12))
def test_signed_edt_random(seed):
    rng = np.random.default_rng(seed)
    h, w = (int(v) for v in rng.integers(1, 25, size=2))
    w = max(w, 2) if h == 1 else w
    m = rng.random((h, w)) < rng.choice([0.05, 0.5, 0.95])
    if m.all() or not m.any():
        m.flat[0] = not m.flat[0]
    u = np.where(m, rng.random((h, w)) + 0.1, -rng.random((h, w)))
    for window in (64, 1):
        d2, un, changed = R.signed_edt(u, window=window)
        assert changed and np.array_equal(d2, R.naive_d2(m))
    rows = [0, h - 1]
    d2r, unr, _ = R.signed_edt(u, rows=rows)
    assert np.array_equal(d2r, d2[rows]) and np.array_equal(R.bits(unr), R.bits(un[rows]))


def test_mask_rule_edges():
    u = np.array([[np.nan, -0.0, 1e-60, -1e-60, 0.0, 1e-45, 1.0, -np.inf, np.inf]])
    assert R.mask_of(u).tolist() == [[False, False, False, False, False, True, True, False, True]]
    # float32's smallest subnormal is 1.4e-45: half of it and below rounds to 0.0f
    assert R.mask_of(np.array([7.1e-46, 7.0e-46])).tolist() == [True, False]


@pytest.mark.parametrize("value", [2.5, -1.0, 0.0, np.nan])
def test_uniform_mask_is_untouched(value):
    u = np.full((5, 7), value)
    u[2, 3] = value * 2 if value == value else value
    d2, un, changed = R.signed_edt(u)
    assert changed is False
    assert np.array_equal(R.bits(un), R.bits(u))


def test_new_symbols_are_exported(capi):
    """Fails on the parent commit: neither the header, nor EXPORTS, nor the library has them."""
    raw = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    for name in ("cvh_reinit", "cvh_reinit_batch"):
        assert name in capi.EXPORTS
        assert hasattr(raw, name)
        assert f"int {name}(" in hdr
    assert hasattr(capi.Context, "reinit") and callable(capi.reinit_batch)
    assert callable(capi.run_with_reinit) and callable(capi.run_batch_with_reinit)


def test_batch_argument_errors_without_device(capi):
    with pytest.raises(capi.CvhError) as e:
        capi.reinit_batch([])
    assert e.value.code == 1 and "cvh_reinit_batch: empty member list" in str(e.value)
    L = capi.lib()
    members = (ctypes.c_void_p * 2)(None, None)
    changed = (ctypes.c_int * 2)(7, 7)
    assert L.cvh_reinit_batch(members, 2, changed) == 1
    assert b"cvh_reinit_batch: member 0 is NULL" in L.cvh_last_error(None)
    assert list(changed) == [7, 7]
    assert L.cvh_reinit_batch(None, 2, None) == 1
    assert L.cvh_reinit_batch(members, -1, None) == 1
    assert L.cvh_reinit(None, None) == 1


class FakeContext:
    def __init__(self, stops_at=None):
        self.calls, self.stops_at, self.done = [], stops_at, 0

    def run(self, max_steps=-1):
        self.calls.append(("run", max_steps))
        k = max_steps
        if self.stops_at is not None and self.done + k >= self.stops_at:
            k = self.stops_at - self.done
            self.stopped = True
        else:
            self.stopped = False
        self.done += k
        return k, 0.25 * self.done

    def sync(self):
        return self.done, 0.0, self.stopped


def test_run_with_reinit_zero_delegates_to_run(capi, monkeypatch):
    for every in (0, -3):
        ctx = FakeContext()
        assert capi.run_with_reinit(ctx, 40, every) == (40, 10.0)
        assert ctx.calls == [("run", 40)]
    seen = []
    monkeypatch.setattr(capi, "run_batch", lambda cs, k: seen.append((cs, k)) or [(1, 2.0), (3, 4.0)])
    assert capi.run_batch_with_reinit(["a", "b"], 17, 0) == [(1, 2.0), (3, 4.0)]
    assert seen == [(["a", "b"], 17)]


def test_run_with_reinit_segments(capi, monkeypatch):
    reinits = []
    monkeypatch.setattr(capi, "reinit_batch", lambda cs: reinits.append(list(cs)) or [True] * len(cs))
    ctx = FakeContext()
    assert capi.run_with_reinit(ctx, 50, 20) == (50, 12.5)
    assert ctx.calls == [("run", 20), ("run", 20), ("run", 10)] and reinits == [[ctx], [ctx]]
    # a stop inside the second segment ends the run there: no reinit follows, no third segment
    del reinits[:]
    ctx = FakeContext(stops_at=27)
    assert capi.run_with_reinit(ctx, 60, 20) == (27, 6.75)
    assert ctx.calls == [("run", 20), ("run", 20)] and reinits == [[ctx]]
    # the batch form drops the stopped member
    del reinits[:]
    a, b = FakeContext(stops_at=20), FakeContext()
    monkeypatch.setattr(capi, "run_batch", lambda cs, k: [c.run(k) for c in cs])
    out = capi.run_batch_with_reinit([a, b], 60, 20)
    assert out == [(20, 5.0), (60, 15.0)]
    assert len(a.calls) == 1 and len(b.calls) == 3 and reinits == [[b], [b]]


def test_cli_rejects_negative_reinit(capi, tmp_path):
    cli = os.path.join(ROOT, "bin", "chan_vese")
    img = tmp_path / "a.pgm"
    with open(img, "wb") as f:
        f.write(b"P5\n8 8\n255\n" + bytes(64))
    r = subprocess.run([cli, "-i", str(img), "--reinit", "-1"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Reinitialisation interval cannot be negative: -1." in r.stderr
    r = subprocess.run([cli, "-i", str(img), "--reinit", "x"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "error: the argument ('x') for option '--reinit' is invalid" in r.stderr
    r = subprocess.run([cli, "-i", str(img), "--reinit", "5", "-V"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "Reinitialisation (--reinit) cannot be combined with video output (-V)." in r.stderr
    assert "--reinit" in subprocess.run([cli, "-h"], capture_output=True, text=True, timeout=120).stdout
