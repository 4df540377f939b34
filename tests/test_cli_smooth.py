"""chan_vese --smooth / --smooth-sigma / --edge-sigma: without a GPU the options are parsed and validated, each refusal with its message,
before any device is touched; --help --verbose lists them and the plain --help does not.  On the GPU (marked): --smooth blur|detail
--dump-planes gives the restatement's planes (smooth_util) behind --rank and in front of --local, and --edge K --edge-sigma S
--dump-edge gives the numpy edge map (geodesic_util) of the blurred plane, byte for byte."""
import numpy as np
import pytest

import geodesic_util as G
import local_util as LU
import rank_util as RU
import smooth_util as U
import cli_util
from cli_util import BIN as CLI, head_comment, write_pgm


def run(*args):
    return cli_util.run(CLI, *args, timeout=120)


def read_pgm_tail(path, h, w):
    return np.frombuffer(open(path, "rb").read()[-h * w:], dtype=np.uint8).reshape(h, w)


@pytest.fixture()
def img(tmp_path):
    path = tmp_path / "a.ppm"
    with open(path, "wb") as f:
        f.write(b"P6\n40 40\n255\n" + bytes(4800))
    return str(path)


def test_smooth_is_validated(img):
    for bad in ("mean", "gauss", "copy", "1"):
        r = run("-i", img, "--smooth", bad)
        assert r.returncode == 1 and "Invalid smoothing requested." in r.stderr and "blur, detail" in r.stderr
    for bad in ("0", "-1", "21.5", "nan", "inf"):
        r = run("-i", img, "--smooth", "blur", "--smooth-sigma", bad)
        assert r.returncode == 1 and "Smoothing scale (--smooth-sigma) must be a finite number > 0 and at most 21" in r.stderr, (bad, r.stderr)
    r = run("-i", img, "--smooth", "blur", "--smooth-sigma", "wide")
    assert r.returncode == 1 and "error: the argument ('wide') for option '--smooth-sigma' is invalid" in r.stderr
    r = run("-i", img, "--smooth-sigma", "2")
    assert r.returncode == 1 and r.stderr.strip() == "A scale (--smooth-sigma) needs a smoothing (--smooth)."
    r = run("-i", img, "--smooth")
    assert r.returncode == 1 and "error: the required argument for option '--smooth' is missing" in r.stderr
    r = run("-i", img, "--smooth", "blur", "--phases", "4")
    assert r.returncode == 1 and "Four phases (--phases 4)" in r.stderr and "--smooth" in r.stderr
    r = run("-i", img, "-g", "--smooth", "detail", "--lambda1", "1", "1", "1")       # a smoothing keeps the channel count
    assert r.returncode == 1 and "Too many lambda1 values for a grayscale image." in r.stderr


def test_edge_sigma_is_validated(img):
    r = run("-i", img, "--edge-sigma", "2")
    assert r.returncode == 1 and r.stderr.strip() == "A blurred edge map (--edge-sigma) needs an edge-weighted run (--edge)."
    for bad in ("0", "-2", "22", "nan"):
        r = run("-i", img, "--edge", "10", "--edge-sigma", bad)
        assert r.returncode == 1 and "Edge scale (--edge-sigma) must be a finite number > 0 and at most 21" in r.stderr, (bad, r.stderr)
    r = run("-i", img, "--edge", "10", "--edge-sigma")
    assert r.returncode == 1 and "error: the required argument for option '--edge-sigma' is missing" in r.stderr
    r = run("-i", img, "--edge", "10", "--edge-sigma", "2", "--levels", "2")        # --edge's own refusals stand
    assert r.returncode == 1 and "Edge-weighted length (--edge)" in r.stderr
    r = run("-i", img, "--edge", "0", "--edge-sigma", "2")
    assert r.returncode == 1 and "Edge contrast (--edge) must be a finite number > 0" in r.stderr


def test_help_lists_the_flags_with_verbose_only():
    plain, verbose = run("-h").stdout, run("-h", "--verbose").stdout
    for flag in ("--smooth arg", "--smooth-sigma arg (=1)", "--edge-sigma arg"):
        assert flag in verbose and flag not in plain
    assert "--smooth" not in plain and "--edge-sigma" not in plain and verbose.startswith(plain) and "blur | detail" in verbose
    assert "--smooth blur|detail" in head_comment() and "--edge-sigma S" in head_comment()


@pytest.mark.gpu
def test_cli_smooth_dumps_the_restatements_planes(tmp_path):
    n = RU.PROP_N
    plane = np.array(RU.salt_image())
    src = tmp_path / "salt.pgm"
    write_pgm(src, plane)
    for what, sigma in (("blur", "1"), ("detail", "2.5"), ("BLUR", "0.5")):
        out = tmp_path / f"{what}.pgm"
        r = run("-i", str(src), "-g", "--smooth", what, "--smooth-sigma", sigma, "-N", "3", "--dump-planes", str(out))
        assert r.returncode == 0, r.stderr
        taps = U.gauss_taps(float(sigma))[1]
        assert np.array_equal(read_pgm_tail(out, n, n), U.expected([plane], 1, taps, (U.NAMES[what.lower()],))[0]), what
    out = tmp_path / "default.pgm"                                                   # --smooth-sigma defaults to 1
    assert run("-i", str(src), "-g", "--smooth", "blur", "-N", "1", "--dump-planes", str(out)).returncode == 0
    assert np.array_equal(read_pgm_tail(out, n, n), U.blur(plane, U.gauss_taps(1.0)[1]))
    # behind --rank and in front of --local
    r = run("-i", str(src), "-g", "--rank", "median", "--rank-radius", "1", "--smooth", "blur", "--smooth-sigma", "1.5", "--local", "stack",
            "--local-radius", "2", "-N", "3", "--dump-planes", str(out))
    assert r.returncode == 0, r.stderr
    smoothed = U.blur(RU.fast(plane, 1, RU.MEDIAN), U.gauss_taps(1.5)[1])
    assert np.array_equal(read_pgm_tail(out, 3 * n, n), np.concatenate(LU.expected([smoothed], 3, 2, LU.STACK), axis=0))


@pytest.mark.gpu
def test_cli_edge_sigma_dumps_the_map_of_the_blurred_plane(tmp_path):
    plane = G.demo_scene()[0]
    h, w = plane.shape
    src, edge, planes = tmp_path / "scene.pgm", tmp_path / "edge.raw", tmp_path / "planes.pgm"
    write_pgm(src, plane)
    r = run("-i", str(src), "-g", "--edge", "15", "--edge-sigma", "2", "--init", "otsu", "-N", "5", "--dump-edge", str(edge), "--dump-planes", str(planes))
    assert r.returncode == 0, r.stderr
    got = np.fromfile(edge, dtype="<u2").reshape(h, w)
    assert np.array_equal(got, G.edge_map([U.blur(plane, U.gauss_taps(2.0)[1])], 15.0))
    assert not np.array_equal(got, G.edge_map([plane], 15.0))
    assert np.array_equal(read_pgm_tail(planes, h, w), plane)                        # the run kept the unblurred plane
