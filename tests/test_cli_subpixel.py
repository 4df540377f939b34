"""bin/chan_vese --contours FILE --contours-subpixel: -h lists it and the refusals hold (CPU); on the GPU the text file of a 64 x 64
synthetic disk parses back into what Context.contours_subpixel() gives for the level set --dump-u writes in the same run."""
import numpy as np
import pytest

from chan_vese_amd import synth
from cli_util import cli, head_comment, run, write_pgm

N = 64


def test_help_and_refusals(cli, tmp_path):
    text = run(cli, "-h").stdout
    assert "--contours-subpixel" in text and "%.17g" in text
    head = head_comment()
    assert "--contours-subpixel" in head and "Subpixel contours" in head
    write_pgm(tmp_path / "a.pgm", synth.disk(N, 190, 60, noise=48, seed=4))
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "--contours-subpixel")
    assert r.returncode != 0 and "Subpixel points (--contours-subpixel) need a contour file (--contours)." in r.stdout + r.stderr
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "--contours", str(tmp_path / "c.txt"), "--contours-subpixel", "--contours-all")
    assert r.returncode != 0
    assert "Subpixel points (--contours-subpixel) cannot be combined with every lattice vertex (--contours-all)." in r.stdout + r.stderr
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "-V", "--contours", str(tmp_path / "c.txt"), "--contours-subpixel")
    assert r.returncode != 0 and "A contour file (--contours) cannot be combined with video output (-V)." in r.stdout + r.stderr
    assert not (tmp_path / "c.txt").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("flags,opts", [([], dict(conn=4)), (["-I", "--connectivity", "8", "--min-area", "3", "--fill-holes", "-1", "--largest"],
                                                             dict(conn=8, invert=True, min_area=3, fill_holes=-1, keep_largest=True))],
                         ids=["raw", "cleaned_inverted"])
def test_file_parses_back_into_the_python_call(cli, tmp_path, flags, opts):
    from chan_vese_amd import capi
    img = synth.disk(N, 190, 60, noise=48, seed=4)
    write_pgm(tmp_path / "a.pgm", img)
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "-t", "0", "-N", "12", "-g", *flags, "--contours", str(tmp_path / "c.txt"), "--contours-subpixel",
            "--dump-u", str(tmp_path / "u.f64"))
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "", (r.stdout, r.stderr)
    u = np.frombuffer((tmp_path / "u.f64").read_bytes(), "<f8").reshape(N, N)
    with capi.Context(N, N, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_levelset(u)
        loops, points = ctx.contours_subpixel(**opts)
    lines = (tmp_path / "c.txt").read_text().splitlines()
    assert len(lines) == loops.size and loops.size >= 1
    assert np.any(points != np.floor(points * 2) / 2)   # (not all of them midpoints or lattice points)
    for l, line in zip(loops, lines):
        head, _, tail = line.partition(" :")
        assert [int(x) for x in head.split()] == [int(l["first"]), int(l["edges"]), int(l["area2"])]
        got = [[float(v) for v in pair.split(",")] for pair in tail.split()]   # (%.17g reads back to the same double)
        assert got == points[int(l["offset"]):int(l["offset"]) + int(l["points"])].tolist()
