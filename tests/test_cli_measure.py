"""bin/chan_vese --measure FILE: -h lists it (CPU); on the GPU the CSV of a small synthetic image parses, its integer columns are the
restatement's (measure_util.py) on the mask --dump-mask writes in the same run, and its doubles are capi.region_shapes' of that table."""
import numpy as np
import pytest

import measure_util as mu
from chan_vese_amd import synth
from cli_util import cli, head_comment, run, write_pgm

H, W = 40, 56
INT_COLS = ["first", "area", "x0", "y0", "x1", "y1", "border", "perimeter"]
DOUBLE_COLS = ["cx", "cy", "mu20", "mu02", "mu11", "theta", "major", "minor"]


def test_help_lists_the_measure_flag(cli):
    text = run(cli, "-h").stdout
    assert "--measure arg" in text and "first,area,x0,y0,x1,y1,border,perimeter,cx,cy,mu20,mu02,mu11,theta,major,minor" in text
    head = head_comment()
    assert "--measure" in head
    r = run(cli, "-i", "x.pgm", "--measure")
    assert r.returncode == 1 and "error: the required argument for option '--measure' is missing" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("grey,flags,conn", [(True, [], 4), (True, ["-I", "--connectivity", "8", "--min-area", "3", "--fill-holes", "-1"], 8),
                                             (False, ["--min-area", "2"], 4)], ids=["raw", "cleaned_inverted", "colour"])
def test_csv_matches_the_restatement(cli, tmp_path, grey, flags, conn):
    from chan_vese_amd import capi
    img = synth.disk(H, 190, 60, noise=48, seed=4, h=H, w=W)
    write_pgm(tmp_path / "a.pgm", img)
    channels = 1 if grey else 3
    base = ["-i", str(tmp_path / "a.pgm"), "-t", "0", "-N", "12"] + (["-g"] if grey else [])
    r = run(cli, *base, *flags, "--measure", str(tmp_path / "m.csv"), "--dump-mask", str(tmp_path / "m.pgm"))
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "", (r.stdout, r.stderr)
    mask = np.frombuffer((tmp_path / "m.pgm").read_bytes()[-H * W:], np.uint8).reshape(H, W) != 0
    want = mu.measure(mask, [img] * channels, conn)   # (a grey file gives three equal planes without -g)
    shapes = capi.region_shapes(want, channels)
    lines = (tmp_path / "m.csv").read_text().splitlines()
    names = ["label"] + INT_COLS + DOUBLE_COLS + [f"mean{k}" for k in range(channels)] + [f"var{k}" for k in range(channels)]
    assert lines[0] == ",".join(names)
    assert len(lines) == 1 + want.size and want.size >= (2 if not flags else 1)   # (the raw noisy mask has speckle beside the disk)
    for k, line in enumerate(lines[1:]):
        cells = dict(zip(names, line.split(",")))
        assert len(line.split(",")) == len(names)
        assert int(cells["label"]) == k + 1
        for f in INT_COLS:
            assert int(cells[f]) == int(want[f][k]), (k, f)
        for f in DOUBLE_COLS:
            assert float(cells[f]) == float(shapes[f][k]), (k, f)
        for j in range(channels):
            assert float(cells[f"mean{j}"]) == float(shapes["mean"][k][j]) and float(cells[f"var{j}"]) == float(shapes["var"][k][j]), (k, j)
