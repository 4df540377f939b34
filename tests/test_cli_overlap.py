"""bin/chan_vese --truth-labels: -h lists it and a label image of another size is refused before any device is touched (CPU); on the GPU the
printed integers are the restatement's (overlap_util.py) for the level set the run leaves, with the cleaning options applied, and mean_ap
is capi.ObjectScore's."""
import math

import numpy as np
import pytest

import components_util as cu
import overlap_util as ou
from cli_util import cli, head_comment, run, write_pgm

H, W = 64, 64
SQUARES = [(6, 8, 1), (10, 40, 2), (38, 20, 300)]   # top, left, label: 16 x 16 each


def planes():
    """the image: three bright squares and a few bright specks on a dark ground; the labels: the squares (the third one shifted by two
    pixels), and a fourth object the image does not show"""
    rng = np.random.default_rng(3)
    img = rng.integers(20, 50, (H, W)).astype(np.uint8)
    labels = np.zeros((H, W), np.int32)
    for k, (top, left, lab) in enumerate(SQUARES):
        img[top:top + 16, left:left + 16] = 200 + 10 * k
        shift = 2 if k == 2 else 0
        labels[top + shift:top + shift + 16, left:left + 16] = lab
    labels[50:60, 50:60] = 65535
    for y, x in ((2, 2), (30, 60), (60, 4)):
        img[y, x] = 230
    return img, labels


def parse(line):
    tok = line.split()
    assert tok[0] == "objects:" and [t.split("=")[0] for t in tok[1:]] == ["objects_a", "objects_b", "tp", "fp", "fn", "mean_ap"], line
    return {k: (float(v) if k == "mean_ap" else int(v)) for k, v in (t.split("=") for t in tok[1:])}


def test_help_lists_the_flag(cli):
    text = run(cli, "-h").stdout
    assert "--truth-labels arg" in text and "objects_a= objects_b= tp= fp= fn= mean_ap=" in text
    head = head_comment()
    assert "--truth-labels" in head


def test_a_label_image_of_another_shape_is_refused(cli, tmp_path):
    img, labels = planes()
    write_pgm(tmp_path / "a.pgm", img)
    write_pgm(tmp_path / "small.pgm", labels[:, :-1], 65535)
    base = ["-i", str(tmp_path / "a.pgm"), "-g"]
    r = run(cli, *base, "--truth-labels", str(tmp_path / "small.pgm"))
    assert r.returncode == 1 and f"is {W - 1} x {H}, the input {W} x {H}: they must have the same size." in r.stderr, r.stderr
    r = run(cli, *base, "--truth-labels", str(tmp_path / "missing.pgm"))
    assert r.returncode == 1 and "missing.pgm" in r.stderr
    (tmp_path / "colour.ppm").write_bytes(b"P6\n%d %d\n255\n" % (W, H) + bytes(3 * H * W))
    r = run(cli, *base, "--truth-labels", str(tmp_path / "colour.ppm"))
    assert r.returncode == 1 and "a label image must be a binary PGM with maxval <= 65535 or an 8-bit grey PNG" in r.stderr
    r = run(cli, *base, "--truth-labels")
    assert r.returncode == 1 and "error: the required argument for option '--truth-labels' is missing" in r.stderr


@pytest.mark.gpu
def test_objects_line_matches_the_restatement(cli, tmp_path):
    from chan_vese_amd import capi
    img, labels = planes()
    write_pgm(tmp_path / "a.pgm", img)
    write_pgm(tmp_path / "wide.pgm", labels, 65535)
    write_pgm(tmp_path / "narrow.pgm", np.minimum(labels, 255))
    base = ["-i", str(tmp_path / "a.pgm"), "-g", "-t", "0", "-N", "24"]
    plain = run(cli, *base, "--dump-u", str(tmp_path / "u0.bin"))
    assert plain.returncode == 0 and plain.stdout == "", (plain.stdout, plain.stderr)
    seen = []
    for name, truth, extra, clean in (("wide.pgm", labels, [], (4, 0, 0, False)), ("narrow.pgm", np.minimum(labels, 255), [], (4, 0, 0, False)),
                                      ("wide.pgm", labels, ["--connectivity", "8", "--min-area", "4"], (8, 4, 0, False))):
        r = run(cli, *base, "--truth-labels", str(tmp_path / name), *extra, "--dump-u", str(tmp_path / "u1.bin"))
        assert r.returncode == 0 and r.stderr == "", r.stderr
        assert (tmp_path / "u0.bin").read_bytes() == (tmp_path / "u1.bin").read_bytes()          # the call only reads
        lines = r.stdout.splitlines()
        assert len(lines) == 1
        got = parse(lines[0])
        u = np.fromfile(tmp_path / "u1.bin", dtype=np.float64).reshape(H, W)
        rows, _ = ou.overlaps(cu.foreground(u), truth, *clean)
        want = ou.match(rows, 1, 2)
        print(lines[0], want[:5])
        assert (got["objects_a"], got["objects_b"], got["tp"], got["fp"], got["fn"]) == want[:5]
        ref = capi.ObjectScore(*want[:5], tuple(ou.match(rows, q, 20)[2] for q in range(10, 20)))
        assert got["mean_ap"] == ref.mean_ap or (math.isnan(got["mean_ap"]) and math.isnan(ref.mean_ap))
        seen.append(want[:5])
    assert seen[0][1] == 4 and seen[0][2] >= 3 and seen[0][4] >= 1   # the three squares are found, the fourth object is missed
    assert seen[2][0] < seen[0][0]                                   # the specks are components until --min-area drops them
