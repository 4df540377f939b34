"""bin/chan_vese --convex TAU[,SIGMA] [--convex-means M] [--convex-stop S]: the options are validated before any device is touched and
--help --verbose lists them (CPU); on the GPU the level set and the mask are the restatement's, plain and with --edge K."""
import numpy as np
import pytest

import convex_util as X
import geodesic_util as G
from cli_util import cli, head_comment, run, write_pgm   # noqa: F401  (cli: the fixture)

H, W = 64, 64


def test_refused_combinations_exit_with_their_message(cli, tmp_path):
    img = tmp_path / "a.pgm"
    write_pgm(img, np.zeros((H, W), dtype=np.uint8))
    base = ["-i", str(img), "-g", "--convex", "0.25"]
    for other, word in ((["--phases", "4"], "four phases (--phases 4)"), (["--localized", "5"], "localised regions (--localized)"),
                        (["--levels", "2"], "a coarse-to-fine run (--levels)"), (["--energy"], "an energy line (--energy)"),
                        (["--energy-every", "4"], "an energy series (--energy-every)"), (["--reinit", "8"], "reinitialisation (--reinit)"),
                        (["-V"], "video output (-V)"), (["--state", "32"], "FP32 state (--state 32)")):
        r = run(cli, *base, *other)
        assert r.returncode == 1 and "Convex relaxation (--convex) cannot be combined with " + word + "." in r.stderr, (other, r.stderr)
    for bad in ("0", "-2", "nan", "inf", "0.25,0", "0.25,nan", "0.5,0.2500001", "1,1"):
        r = run(cli, "-i", str(img), "-g", "--convex", bad)
        assert r.returncode == 1 and "Convex steps (--convex TAU[,SIGMA]) must be finite numbers > 0 with 8 TAU SIGMA <= 1" in r.stderr, (bad, r.stderr)
    for bad in ("x", "0.25,", "0.25;0.5"):
        r = run(cli, "-i", str(img), "-g", "--convex", bad)
        assert r.returncode == 1 and "for option '--convex' is invalid" in r.stderr, (bad, r.stderr)
    r = run(cli, *base, "--convex-means", "-1")
    assert r.returncode == 1 and "Means interval (--convex-means) cannot be negative: -1." in r.stderr, r.stderr
    r = run(cli, *base, "--convex-stop", "nan")
    assert r.returncode == 1 and "Stop level (--convex-stop) must be a number" in r.stderr, r.stderr
    for alone in (["--convex-means", "2"], ["--convex-stop", "0.1"]):
        r = run(cli, "-i", str(img), "-g", *alone)
        assert r.returncode == 1 and "need a convex run (--convex)." in r.stderr, r.stderr


def test_verbose_help_lists_the_options_and_plain_help_does_not(cli):
    plain, verbose = run(cli, "-h").stdout, run(cli, "-h", "--verbose").stdout
    assert "--convex" not in plain
    assert verbose.startswith(plain)
    for flag in ("--convex arg", "--convex-means arg (=1)", "--convex-stop arg (=0)", "8 TAU SIGMA <= 1"):
        assert flag in verbose, flag
    assert "--convex TAU[,SIGMA]" in head_comment() and "--convex-means" in head_comment() and "--convex-stop" in head_comment()


def read_outputs(tmp_path):
    u = np.frombuffer((tmp_path / "u.bin").read_bytes(), dtype=np.float64).reshape(H, W)
    pgm = (tmp_path / "m.pgm").read_bytes()
    assert pgm.startswith(b"P5")
    return u, np.frombuffer(pgm[-H * W:], dtype=np.uint8).reshape(H, W)


@pytest.mark.gpu
def test_the_disk_run_is_the_restatement(cli, tmp_path):
    """defaults of --convex-means and --convex-stop: the noisy disk stops at its exact fixed point, where the restatement stops"""
    img, _ = X.disk_scene()
    write_pgm(tmp_path / "a.pgm", img)
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "-g", "--math", "strict", "-N", "64", "--lambda1", "0.001", "--lambda2", "0.001", "--convex", "0.25",
            "--verbose", "--dump-u", str(tmp_path / "u.bin"), "--dump-mask", str(tmp_path / "m.pgm"))
    assert r.returncode == 0, (r.stdout, r.stderr)
    rv, rsteps, _ = X.disk_reference()
    u, m = read_outputs(tmp_path)
    assert np.array_equal(u, rv - 0.5) and np.array_equal(m, X.mask(rv - 0.5) * 255)
    assert f"{rsteps} iterations" in r.stderr or f" {rsteps} " in r.stderr, r.stderr


@pytest.mark.gpu
def test_steps_means_stop_and_edge_reach_the_library(cli, tmp_path):
    """TAU,SIGMA, --convex-means 2, --convex-stop -1, --init otsu and --edge K: 12 iterations of the weighted model on the noisy scene (b)
    of the demonstration -- a third of its pixels are still strictly between 0 and 1 then, the run is no threshold --, as the restatement"""
    img, _ = X.hard_scene()
    write_pgm(tmp_path / "a.pgm", img)
    steps = 12
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "-g", "-N", str(steps), "--mu", "0.5", "--lambda1", "0.0001", "--lambda2", "0.0001", "--init", "otsu",
            "--edge", "30", "--convex", "0.5,0.125", "--convex-means", "2", "--convex-stop", "-1", "--dump-edge", str(tmp_path / "g.bin"),
            "--dump-u", str(tmp_path / "u.bin"), "--dump-mask", str(tmp_path / "m.pgm"))
    assert r.returncode == 0, (r.stdout, r.stderr)
    gq = G.edge_map([img], 30.0)
    assert (tmp_path / "g.bin").read_bytes() == gq.tobytes()
    u0, _ = G.demo_start(img)
    p = dict(mu=0.5, nu=0.0, lambda1=(1e-4,) * 3, lambda2=(1e-4,) * 3, tau=0.5, sigma=0.125, means_every=2)
    st, done, _ = X.run([img], u0, gq, p, steps)
    u, m = read_outputs(tmp_path)
    e = np.abs(u - (st["v"] - 0.5)).max()
    between = float(((st["v"] > 0) & (st["v"] < 1)).mean())
    keep = np.abs(st["v"] - 0.5) >= 1e-6
    print("level set", e, "share of 0 < v < 1", between, "pixels within 1e-6 of 1/2", int((~keep).sum()))
    assert done == steps and e <= 1e-9 and between > 0.01
    assert np.array_equal(m[keep], (X.mask(st["v"] - 0.5) * 255)[keep])
