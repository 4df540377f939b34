"""bin/chan_vese --phases 4: the options are validated before any device is touched and -h lists them (CPU); on the GPU --dump-labels
writes the bytes the capi path gives, -s the label plane times 85, and a run without --phases writes what the parent's program wrote for
an existing CLI case (test_cli_energy.py's: the level set capi leaves for the same run, bit for bit, and nothing on stdout)."""
import numpy as np
import pytest

import multiphase_util as M
from cli_util import cli, head_comment, read_pnm as read_pgm, run, write_pgm

H, W = 40, 56


def test_refused_combinations_exit_with_their_message(cli, tmp_path):
    img = tmp_path / "a.pgm"
    write_pgm(img, np.zeros((H, W), dtype=np.uint8))
    base = ["-i", str(img), "-g", "--phases", "4"]
    for other, word in ((["-V"], "video output (-V)"), (["--levels", "2"], "a coarse-to-fine run (--levels)"), (["--energy"], "an energy line (--energy)"),
                        (["--energy-every", "4"], "an energy series (--energy-every)"), (["--reinit", "8"], "reinitialisation (--reinit)"),
                        (["--dump-u", str(tmp_path / "u.bin")], "--dump-u"), (["--rect", "1,1,4,4"], "--rect")):
        r = run(cli, *base, *other)
        assert r.returncode == 1 and "Four phases (--phases 4) cannot be combined with " + word + "." in r.stderr, (other, r.stderr)
    r = run(cli, "-i", str(img), "-g", "--phases", "3")
    assert r.returncode == 1 and "Number of phases must be 2 or 4: 3." in r.stderr
    r = run(cli, "-i", str(img), "-g", "--init2", "otsu")
    assert r.returncode == 1 and "A second start (--init2) needs four phases (--phases 4)." in r.stderr
    r = run(cli, "-i", str(img), "-g", "--dump-labels", str(tmp_path / "l.bin"))
    assert r.returncode == 1 and "A label file (--dump-labels) needs four phases (--phases 4)." in r.stderr
    r = run(cli, *base, "--init2", "spiral")
    assert r.returncode == 1 and "error: the argument ('spiral') for option '--init2' is invalid" in r.stderr
    r = run(cli, *base, "--init2", "threshold")
    assert r.returncode == 1 and "A threshold start (--init2 threshold T) needs its threshold." in r.stderr
    r = run(cli, *base, "--init2", "threshold", "300")
    assert r.returncode == 1 and "Threshold must be between 0 and 255: 300." in r.stderr
    assert not (tmp_path / "u.bin").exists() and not (tmp_path / "l.bin").exists()


def test_help_lists_the_options(cli):
    text = run(cli, "-h").stdout
    assert "--phases arg (=2)" in text and "--init2 arg (=checkerboard)" in text and "--dump-labels arg" in text
    head = head_comment()
    assert "--phases" in head and "--init2" in head and "--dump-labels" in head


@pytest.mark.gpu
def test_labels_are_the_capi_path(cli, tmp_path):
    from chan_vese_amd import capi
    img = M.disks_image(H, W, 1)[0][0]
    write_pgm(tmp_path / "a.pgm", img)
    base = ["-i", str(tmp_path / "a.pgm"), "-g", "-t", "0", "-N", "10"]

    def capi_labels(start_b):
        with capi.Context(H, W, 1, capi.make_params(tol=0.0)) as a, capi.Context(H, W, 1, capi.make_params(tol=0.0)) as b:
            a.set_image([img])
            b.set_image([img])
            a.init_checkerboard()
            start_b(b)
            assert capi.multiphase_run(a, b, 10)[0] == 10
            return a.multiphase_labels_with(b)

    r = run(cli, *base, "--phases", "4", "--dump-labels", str(tmp_path / "l.bin"), "-s")
    assert r.returncode == 0 and r.stdout == "" and r.stderr == "", (r.stdout, r.stderr)
    want = capi_labels(lambda b: b.set_levelset(np.roll(capi.checkerboard_host(H, W), (2, 3), axis=(0, 1))))
    assert (tmp_path / "l.bin").read_bytes() == want.tobytes()
    assert np.array_equal(read_pgm(tmp_path / "a_selection.pgm"), want * 85)
    r = run(cli, *base, "--phases", "4", "--init2", "threshold", "120", "--dump-labels", str(tmp_path / "l2.bin"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "l2.bin").read_bytes() == capi_labels(lambda b: b.init_threshold(120)).tobytes()
    r = run(cli, *base, "--phases", "4", "--init2", "otsu", "--dump-labels", str(tmp_path / "l3.bin"))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "l3.bin").read_bytes() == capi_labels(lambda b: b.init_otsu()).tobytes()
    # without --phases, and with --phases 2: what the program wrote before the option existed -- the two-phase run's level set, which is
    # capi's for the same run bit for bit (the existing case of test_cli_energy.py), and nothing on stdout
    plain = run(cli, *base, "--dump-u", str(tmp_path / "u0.bin"))
    two = run(cli, *base, "--phases", "2", "--dump-u", str(tmp_path / "u1.bin"))
    assert plain.returncode == 0 and plain.stdout == "" and plain.stderr == "" and two.returncode == 0
    with capi.Context(H, W, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([img])
        ctx.init_checkerboard()
        assert ctx.run(10)[0] == 10
        assert (tmp_path / "u0.bin").read_bytes() == ctx.get_levelset().tobytes() == (tmp_path / "u1.bin").read_bytes()
