"""bin/chan_vese --contours FILE: -h lists it and the refusals hold (CPU); on the GPU the text file of a small synthetic image parses back
into the restatement's loops and points (contour_util.py) of the mask --dump-mask writes in the same run."""
import numpy as np
import pytest

import contour_util as ct
from chan_vese_amd import synth
from cli_util import cli, head_comment, run, write_pgm

H, W = 40, 56


def test_help_and_refusals(cli, tmp_path):
    text = run(cli, "-h").stdout
    assert "--contours arg" in text and "'first edges area2 :'" in text and "--contours-all" in text
    head = head_comment()
    assert "--contours" in head
    r = run(cli, "-i", "x.pgm", "--contours")
    assert r.returncode == 1 and "error: the required argument for option '--contours' is missing" in r.stderr
    write_pgm(tmp_path / "a.pgm", synth.disk(H, 190, 60, noise=48, seed=4, h=H, w=W))
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "-V", "--contours", str(tmp_path / "c.txt"))
    assert r.returncode != 0 and "A contour file (--contours) cannot be combined with video output (-V)." in r.stdout + r.stderr
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "--contours-all")
    assert r.returncode != 0 and "Every lattice vertex (--contours-all) needs a contour file (--contours)." in r.stdout + r.stderr
    assert not (tmp_path / "c.txt").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("flags,conn,simplify", [([], 4, True), (["--contours-all", "--connectivity", "8"], 8, False),
                                                 (["-I", "--connectivity", "8", "--min-area", "3", "--fill-holes", "-1", "--largest"], 8, True)],
                         ids=["raw", "all_vertices", "cleaned_inverted"])
def test_file_parses_back_into_the_restatement(cli, tmp_path, flags, conn, simplify):
    img = synth.disk(H, 190, 60, noise=48, seed=4, h=H, w=W)
    write_pgm(tmp_path / "a.pgm", img)
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "-t", "0", "-N", "12", "-g", *flags, "--contours", str(tmp_path / "c.txt"), "--dump-mask",
            str(tmp_path / "m.pgm"))
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "", (r.stdout, r.stderr)
    mask = np.frombuffer((tmp_path / "m.pgm").read_bytes()[-H * W:], np.uint8).reshape(H, W) != 0
    loops, points = ct.trace(mask, conn, simplify)
    lines = (tmp_path / "c.txt").read_text().splitlines()
    assert len(lines) == loops.size and loops.size >= 1
    for l, line in zip(loops, lines):
        head, _, tail = line.partition(" :")
        assert [int(x) for x in head.split()] == [int(l["first"]), int(l["edges"]), int(l["area2"])]
        got = [[int(v) for v in pair.split(",")] for pair in tail.split()]
        assert got == points[int(l["offset"]):int(l["offset"]) + int(l["points"])].tolist()
