"""bin/chan_vese --edge K [--dump-edge FILE]: the options are validated before any device is touched and --help --verbose lists them
(CPU); on the GPU --dump-edge writes the restatement's bytes of the Perona-Malik-smoothed plane and the mask is the restatement's."""
import numpy as np
import pytest

import geodesic_util as G
from cli_util import cli, run, write_pgm

H, W = 64, 64


def test_refused_combinations_exit_with_their_message(cli, tmp_path):
    img = tmp_path / "a.pgm"
    write_pgm(img, np.zeros((H, W), dtype=np.uint8))
    base = ["-i", str(img), "-g", "--edge", "30"]
    for other, word in ((["--phases", "4"], "four phases (--phases 4)"), (["--localized", "5"], "localised regions (--localized)"),
                        (["--levels", "2"], "a coarse-to-fine run (--levels)"), (["--energy"], "an energy line (--energy)"),
                        (["--energy-every", "4"], "an energy series (--energy-every)"), (["--reinit", "8"], "reinitialisation (--reinit)"),
                        (["-V"], "video output (-V)"), (["--state", "32"], "FP32 state (--state 32)")):
        r = run(cli, *base, *other)
        assert r.returncode == 1 and "Edge-weighted length (--edge) cannot be combined with " + word + "." in r.stderr, (other, r.stderr)
    for bad in ("0", "-2", "nan", "inf"):
        r = run(cli, "-i", str(img), "-g", "--edge", bad)
        assert r.returncode == 1 and "Edge contrast (--edge) must be a finite number > 0" in r.stderr, (bad, r.stderr)
    r = run(cli, "-i", str(img), "-g", "--dump-edge", str(tmp_path / "g.bin"))
    assert r.returncode == 1 and "An edge map file (--dump-edge) needs an edge-weighted run (--edge)." in r.stderr, r.stderr


def test_verbose_help_lists_the_options_and_plain_help_does_not(cli):
    plain, verbose = run(cli, "-h").stdout, run(cli, "-h", "--verbose").stdout
    assert "--edge arg" not in plain and "--dump-edge" not in plain
    assert verbose.startswith(plain) and "--edge arg" in verbose and "--dump-edge arg" in verbose


@pytest.mark.gpu
def test_edge_map_and_mask_are_the_restatement(cli, tmp_path):
    img, _, _ = G.demo_scene()
    write_pgm(tmp_path / "a.pgm", img)
    K, L, T = G.DEMO_PM
    steps = 12
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "-g", "-S", "-K", str(K), "-L", str(L), "-T", str(T), "-t", "0", "-N", str(steps), "--mu", "5",
            "--lambda1", "0.001", "--lambda2", "0.001", "--init", "otsu", "--edge", "30", "--dump-edge", str(tmp_path / "g.bin"),
            "--dump-u", str(tmp_path / "u.bin"), "--dump-mask", str(tmp_path / "m.pgm"))
    assert r.returncode == 0, (r.stdout, r.stderr)
    smooth = G.demo_smoothed(img)
    gq = G.edge_map([smooth], 30.0)
    assert (tmp_path / "g.bin").read_bytes() == gq.tobytes()                  # built after the Perona-Malik stage
    u0, _ = G.demo_start(smooth)                                              # (Otsu sees the smoothed plane too)
    ref = G.run([smooth], u0, gq, G.demo_params(5.0), steps)[0]
    u = np.frombuffer((tmp_path / "u.bin").read_bytes(), dtype=np.float64).reshape(H, W)
    e = np.abs(u - ref).max() / max(1.0, np.abs(ref).max())
    keep = np.abs(ref) >= 1e-6
    print("level set", e, "pixels within 1e-6 of the front", int((~keep).sum()))
    assert e <= 1e-9 and (~keep).mean() <= 1e-3
    pgm = (tmp_path / "m.pgm").read_bytes()
    m = np.frombuffer(pgm[-H * W:], dtype=np.uint8).reshape(H, W)
    assert pgm.startswith(b"P5") and np.array_equal(m[keep], (G.mask(ref) * 255)[keep])
