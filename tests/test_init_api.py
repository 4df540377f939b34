"""Device-side initial level sets without a GPU: the restated Otsu (init_util.otsu) against an exact-rational maximum, the library's
host helper cvh_otsu_from_histogram against the restatement (128-bit d, ties, degenerate histograms), the exported symbols, the argument
errors a call can decide before it touches a device, the Python helpers, Segmenter's validation of `init` and the CLI's of its options."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import init_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cvh_histogram", "cvh_histogram_batch", "cvh_otsu_from_histogram", "cvh_otsu_threshold", "cvh_init_threshold", "cvh_init_threshold_batch",
       "cvh_init_otsu", "cvh_init_otsu_batch", "cvh_init_rect", "cvh_init_rect_batch", "cvh_init_disk", "cvh_init_disk_batch"]


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi
    return capi


ALL_HISTS = {**U.histograms_for_otsu(), **U.huge_histograms()}


@pytest.mark.parametrize("name", sorted(ALL_HISTS))
def test_restated_otsu_is_the_exact_maximum(name):
    """float(d) * float(d) / float(q) carries three roundings (2^-53 each, and the square doubles the first): the candidate it picks has
    an EXACT score within 1e-12 relative of the exact maximum."""
    hist = ALL_HISTS[name]
    t = U.otsu(hist)
    t_exact, best = U.otsu_exact(hist)
    got = U.exact_score(hist, t)
    assert best > 0 and got is not None
    assert abs(got - best) <= Fraction(1, 10 ** 12) * best, (t, t_exact)
    assert t <= t_exact or got < best            # ties go to the smallest t


def test_restated_pieces():
    planes = U.planes_of("ramp", 33, 47, 3)
    assert np.array_equal(U.histogram(planes), np.ones(766) * 2 + (np.arange(766) < 33 * 47 - 2 * 766))
    assert U.grey(planes).max() == 765 and all(p.dtype == np.uint8 for p in planes)
    assert U.histogram(U.planes_of("all255", 4, 5, 3))[765] == 20 and U.histogram(U.planes_of("all0", 4, 5, 1))[0] == 20
    r = U.start_rect(5, 7, -2, 3, 4, 9, 1.0, 0.0)
    assert r.sum() == 2 * 2 and r[3:, :2].all()
    d = U.start_disk(5, 7, 3, 2, 1, 2.0, -1.0)
    assert (d == 2.0).sum() == 5 and d[2, 3] == 2.0 and d[1, 2] == -1.0
    assert (U.start_disk(5, 7, 3, 2, 0, 1.0, 0.0) == 1.0).sum() == 1
    nan = U.start_threshold([np.array([[1, 9]], dtype=np.uint8)], 5, np.nan, 3.0)
    assert np.isnan(nan[0, 1]) and nan[0, 0] == 3.0


@pytest.mark.parametrize("name", sorted(ALL_HISTS))
def test_library_otsu_equals_the_restatement(capi, name):
    """Fails on the parent commit: the symbol does not exist."""
    assert capi.otsu_from_histogram(ALL_HISTS[name]) == U.otsu(ALL_HISTS[name])


def test_huge_counts_need_128_bits():
    """the cases meant to exercise 128-bit d really do: |d| passes 2^64 for some candidate"""
    for name, hist in U.huge_histograms().items():
        assert max(abs(d) for _, d, _ in U.otsu_terms(hist)) >= 2 ** 64, name


@pytest.mark.parametrize("name", sorted(U.degenerate_histograms()))
def test_library_otsu_ties_and_single_bins(capi, name):
    hist, t = U.degenerate_histograms()[name]
    assert U.otsu(hist) == t
    assert capi.otsu_from_histogram(hist) == t


def test_library_otsu_on_random_sparse_histograms(capi):
    rng = np.random.default_rng(7)
    for _ in range(200):
        B = int(rng.choice([1, 2, 3, 256, 766]))
        hist = np.zeros(B, dtype=np.uint32)
        k = int(rng.integers(1, min(B, 6) + 1))
        hist[rng.choice(B, k, replace=False)] = rng.integers(1, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
        assert capi.otsu_from_histogram(hist) == U.otsu(hist)


def test_new_symbols_are_exported(capi):
    """Fails on the parent commit: neither the header, nor EXPORTS, nor the library has them."""
    raw = ctypes.CDLL(capi.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    for name in NEW:
        assert name in capi.EXPORTS
        assert hasattr(raw, name)
        assert f"int {name}(" in hdr
    for name in ("histogram", "otsu_threshold", "init_threshold", "init_otsu", "init_rect", "init_disk"):
        assert callable(getattr(capi.Context, name))
    for name in ("histogram_batch", "init_threshold_batch", "init_otsu_batch", "init_rect_batch", "init_disk_batch", "otsu_from_histogram"):
        assert callable(getattr(capi, name))


def test_argument_errors_without_device(capi):
    L = capi.lib()
    ip = ctypes.POINTER(ctypes.c_int)
    members = (ctypes.c_void_p * 2)(None, None)
    ints = (ctypes.c_int * 8)(*([7] * 8))
    ptrs = (ctypes.c_void_p * 2)(None, None)
    batch = {
        "cvh_histogram_batch": lambda m, n: L.cvh_histogram_batch(m, n, ptrs, ints),
        "cvh_init_threshold_batch": lambda m, n: L.cvh_init_threshold_batch(m, n, ints, 1.0, -1.0),
        "cvh_init_otsu_batch": lambda m, n: L.cvh_init_otsu_batch(m, n, ints, 1.0, -1.0),
        "cvh_init_rect_batch": lambda m, n: L.cvh_init_rect_batch(m, n, ints, 1.0, 0.0),
        "cvh_init_disk_batch": lambda m, n: L.cvh_init_disk_batch(m, n, ints, 1.0, 0.0),
    }
    for name, call in batch.items():
        assert call(members, 2) == 1
        assert f"{name}: member 0 is NULL".encode() in L.cvh_last_error(None)
        assert call(None, 2) == 1
        assert f"{name}: empty member list".encode() in L.cvh_last_error(None)
        assert call(members, 0) == 1 and call(members, -1) == 1
    assert list(ints) == [7] * 8
    assert L.cvh_histogram(None, None, 0, None) == 1
    assert L.cvh_otsu_threshold(None, ctypes.cast(ints, ip)) == 1
    assert L.cvh_init_threshold(None, 3, 1.0, -1.0) == 1
    assert L.cvh_init_otsu(None, None, 1.0, -1.0) == 1
    assert L.cvh_init_rect(None, 0, 0, 4, 4, 1.0, 0.0) == 1
    assert L.cvh_init_disk(None, 0, 0, 4, 1.0, 0.0) == 1
    # the host-only helper
    hist = np.array([1, 0, 2], dtype=np.uint32)
    t = ctypes.c_int(-5)
    assert L.cvh_otsu_from_histogram(None, 3, ctypes.byref(t)) == 1
    assert L.cvh_otsu_from_histogram(hist.ctypes.data, 3, None) == 1
    assert L.cvh_otsu_from_histogram(hist.ctypes.data, 0, ctypes.byref(t)) == 1
    assert L.cvh_otsu_from_histogram(hist.ctypes.data, 767, ctypes.byref(t)) == 1
    assert b"bins must be in 1 .. 766" in L.cvh_last_error(None)
    zeros = np.zeros(256, dtype=np.uint32)
    assert L.cvh_otsu_from_histogram(zeros.ctypes.data, 256, ctypes.byref(t)) == 1
    assert b"the histogram is empty" in L.cvh_last_error(None) and t.value == -5
    with pytest.raises(capi.CvhError) as e:
        capi.otsu_from_histogram(zeros)
    assert e.value.code == 1
    with pytest.raises(capi.CvhError) as e:
        capi.init_otsu_batch([])
    assert e.value.code == 1 and "cvh_init_otsu_batch: empty member list" in str(e.value)


class FakeLib:
    """records the calls the module-level helpers make"""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


class FakeContext:
    def __init__(self, channels=1):
        self._h, self.channels = ctypes.c_void_p(1), channels


def test_python_helpers_delegate(capi, monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(capi, "lib", lambda: fake)
    cs = [FakeContext(1), FakeContext(3), FakeContext(1)]
    capi.init_rect_batch(cs, (1, 2, 3, 4), inside=2.0)
    name, args = fake.calls[-1]
    assert name == "cvh_init_rect_batch" and args[1] == 3 and list(args[2]) == [1, 2, 3, 4] * 3 and args[3:] == (2.0, 0.0)
    capi.init_rect_batch(cs, [(1, 2, 3, 4), (5, 6, 7, 8), (9, 10, 11, 12)])
    assert list(fake.calls[-1][1][2]) == list(range(1, 13))
    capi.init_disk_batch(cs, [(1, 2, 3), (4, 5, 6), (7, 8, 0)], 1.0, -1.0)
    name, args = fake.calls[-1]
    assert name == "cvh_init_disk_batch" and list(args[2]) == [1, 2, 3, 4, 5, 6, 7, 8, 0] and args[3:] == (1.0, -1.0)
    capi.init_threshold_batch(cs, 100)
    name, args = fake.calls[-1]
    assert name == "cvh_init_threshold_batch" and list(args[2]) == [100] * 3 and args[3:] == (1.0, -1.0)
    capi.init_threshold_batch(cs, [1, 2, 3])
    assert list(fake.calls[-1][1][2]) == [1, 2, 3]
    assert capi.init_otsu_batch(cs, 3.0, 4.0) == [0, 0, 0]
    name, args = fake.calls[-1]
    assert name == "cvh_init_otsu_batch" and args[1] == 3 and args[3:] == (3.0, 4.0)
    out = capi.histogram_batch(cs, [256, 0, 10])
    name, args = fake.calls[-1]
    assert name == "cvh_histogram_batch" and list(args[3]) == [256, 0, 10] and [o.size for o in out] == [256, 0, 10] and args[2][1] is None
    assert [o.size for o in capi.histogram_batch(cs)] == [256, 766, 256]
    for bad in (lambda: capi.init_rect_batch(cs, [(1, 2, 3, 4)]), lambda: capi.init_rect_batch(cs, (1, 2, 3)),
                lambda: capi.init_disk_batch(cs, [(1, 2, 3, 4)] * 3), lambda: capi.init_threshold_batch(cs, [1, 2]),
                lambda: capi.histogram_batch(cs, [1])):
        n = len(fake.calls)
        with pytest.raises(ValueError):
            bad()
        assert len(fake.calls) == n


def test_segmenter_validates_init_without_a_gpu(capi):
    import torch
    from chan_vese_amd import torch_io
    n = 3
    assert torch_io.check_init("checkerboard", n) == ("checkerboard", None)
    assert torch_io.check_init("otsu", n) == ("otsu", None)
    assert torch_io.check_init(("threshold", 7), n) == ("threshold", [7] * 3)
    assert torch_io.check_init(("threshold", [1, 2, 765]), n, 3) == ("threshold", [1, 2, 765])
    assert torch_io.check_init(("rect", (1, 2, 3, 4)), n) == ("rect", [(1, 2, 3, 4)] * 3)
    assert torch_io.check_init(("rect", [(1, 2, 3, 4), [5, 6, 7, 8], (-9, -1, 1, 1)]), n)[1] == [(1, 2, 3, 4), (5, 6, 7, 8), (-9, -1, 1, 1)]
    assert torch_io.check_init(("disk", (5, 5, 0)), n) == ("disk", [(5, 5, 0)] * 3)
    bad = ["Otsu", "", ("otsu",), ("threshold",), ("threshold", 1, 2), ("threshold", 1.5), ("threshold", True), ("threshold", [1, 2]),
           ("threshold", -1), ("threshold", 256), ("threshold", (1, 2, 3)), ("rect", (1, 2, 3)), ("rect", (1, 2, 0, 4)), ("rect", (1, 2, 3, -4)),
           ("rect", [(1, 2, 3, 4)] * 2), ("rect", (1, 2, 3, 4.0)), ("rect", 5), ("disk", (1, 2)), ("disk", (1, 2, -1)), ("disk", [(1, 2, 3)] * 4),
           ("circle", (1, 2, 3)), (1, 2), ("disk", None)]
    for init in bad:
        with pytest.raises(ValueError):
            torch_io.check_init(init, n, 1)
    assert torch_io.check_init(("threshold", 256), n, 3)[1] == [256] * 3
    # segment() itself refuses them before it looks at the images or calls the library: a Segmenter without contexts suffices
    seg = object.__new__(torch_io.Segmenter)
    seg.n, seg.h, seg.w, seg.channels, seg.device, seg.contexts, seg.thresholds = n, 8, 8, 1, 0, [], None
    images = torch.zeros((n, 8, 8), dtype=torch.uint8)
    for init in bad:
        with pytest.raises(ValueError, match="init"):
            seg.segment(images, init=init)
    with pytest.raises(ValueError, match="images lives on"):
        seg.segment(images, init="otsu")                 # a good start: the next check is the images'
    with pytest.raises(ValueError):
        seg.segment(images, init=[1, 2, 3])              # neither text, tuple nor tensor: the existing error


def test_cli_validates_the_new_options(capi, tmp_path):
    cli = os.path.join(ROOT, "bin", "chan_vese")
    img = tmp_path / "a.pgm"
    with open(img, "wb") as f:
        f.write(b"P5\n8 8\n255\n" + bytes(64))

    def run(*args):
        return subprocess.run([cli, "-i", str(img), *args], capture_output=True, text=True, timeout=120)

    pairs = [(["--rect", "1,1,4,4"], "--rect"), (["--circ", "4,4,2"], "--circ"), (["--disk", "4,4,2"], "--disk"), (["--init", "otsu"], "--init otsu"),
             (["--threshold", "9"], "--threshold")]
    for i, (a, na) in enumerate(pairs):
        for b, nb in pairs[i + 1:]:
            r = run(*a, *b)
            assert r.returncode == 1 and "Cannot initialize with both" in r.stderr, (a, b, r.stderr)
            if (na, nb) != ("--rect", "--circ"):
                assert f"Cannot initialize with both {na} and {nb}" in r.stderr
    r = run("--init", "sobel")
    assert r.returncode == 1 and "error: the argument ('sobel') for option '--init' is invalid" in r.stderr
    r = run("--threshold", "x")
    assert r.returncode == 1 and "error: the argument ('x') for option '--threshold' is invalid" in r.stderr
    r = run("-g", "--threshold", "256")
    assert r.returncode == 1 and "Threshold must be between 0 and 255: 256." in r.stderr
    r = run("--threshold", "766")
    assert r.returncode == 1 and "Threshold must be between 0 and 765: 766." in r.stderr
    r = run("--threshold", "-1")
    assert r.returncode == 1 and "Threshold must be between 0 and 765: -1." in r.stderr
    for bad in ("4,4", "4,4,-1", "a,b,c", "4,4,2,9", "4,4,2x", ",,"):
        r = run("--disk=" + bad)
        assert r.returncode == 1 and "You must specify the disk as cx,cy,r with a radius that is not negative" in r.stderr, bad
    r = run("--disk")
    assert r.returncode == 1 and "error: the required argument for option '--disk' is missing" in r.stderr
    help_text = subprocess.run([cli, "-h"], capture_output=True, text=True, timeout=120).stdout
    for opt in ("--disk cx,cy,r", "--init arg (=checkerboard)", "--threshold T", "--rect x,y,w,h"):
        assert opt in help_text
    top = open(os.path.join(ROOT, "chan_vese_amd", "host", "main.cpp")).read().split("#include")[0]
    for opt in ("--disk", "--init", "--threshold"):
        assert opt in top
