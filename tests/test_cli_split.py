"""bin/chan_vese --split / --split-labels: --help --verbose lists them (the plain --help is pinned byte for byte by
tests/golden/cli_refusals.json), and bad arguments exit non-zero with a message before any device is touched (CPU); on the GPU `--split 9`
behind `--init-mask` of the demonstration scene with `-N 0` writes the restatement's labels (split_util.py), and --dump-mask, --roi,
--measure, --contours and --truth-labels speak of the split objects, with and without a cleaning option."""
import numpy as np
import pytest

import components_util as CU
import contour_util as CT
import split_util as S
from cli_util import cli, head_comment, read_pnm as read_pgm, run, write_pgm  # noqa: F401

H = W = 64


def test_help_lists_the_split_flags(cli):
    text = run(cli, "-h", "--verbose").stdout
    assert text.startswith(run(cli, "-h").stdout) and "Later additions:" in text
    assert "--split arg" in text and "--split-labels arg" in text and "raw little-endian int32 (h*w)" in text and "--phases 4" in text.split("--split arg")[1]
    head = head_comment()
    assert "--split" in head and "--split-labels" in head


def test_split_flags_are_validated(cli, tmp_path):
    write_pgm(tmp_path / "a.pgm", np.zeros((H, W), dtype=np.uint8))
    base = ["-i", str(tmp_path / "a.pgm"), "-g"]
    for args, text in (
            (["--split", "-1"], "Split radius must be a finite number >= 0."),
            (["--split", "nan"], "Split radius must be a finite number >= 0."),
            (["--split"], "error: the required argument for option '--split' is missing"),
            (["--split-labels", str(tmp_path / "l.bin")], "A split label file (--split-labels) needs an object split (--split)."),
            (["--split", "3", "--morph", "open"], "An object split (--split) cannot be combined with --morph."),
            (["--split", "3", "--phases", "4"], "Four phases (--phases 4) cannot be combined with an object split (--split).")):
        r = run(cli, *base, *args)
        assert r.returncode == 1 and text in r.stderr, (args, r.returncode, r.stderr)
    assert not (tmp_path / "l.bin").exists()


@pytest.mark.gpu
def test_split_applies_to_what_the_mask_outputs_write(cli, tmp_path):
    d = S.demonstration()
    write_pgm(tmp_path / "a.pgm", np.where(d, 200, 50).astype(np.uint8))
    write_pgm(tmp_path / "start.pgm", d.astype(np.uint8))
    base = ["-i", str(tmp_path / "a.pgm"), "-g", "-N", "0", "--init-mask", str(tmp_path / "start.pgm")]
    for clean, f0 in (([], d), (["--min-area", "10"], CU.clean(d, 4, 10, 0, False).astype(bool))):
        want = S.Split(f0, 4, 81)
        assert want.K == (4 if not clean else 3)
        write_pgm(tmp_path / "truth.pgm", (want.labels * want.pieces).astype(np.uint8))
        r = run(cli, *base, *clean, "--split", "9", "--split-labels", str(tmp_path / "l.bin"), "--dump-mask", str(tmp_path / "m.pgm"),
                "--dump-u", str(tmp_path / "u.bin"), "--roi", "--measure", str(tmp_path / "m.csv"), "--contours", str(tmp_path / "c.txt"),
                "--truth-labels", str(tmp_path / "truth.pgm"))
        assert r.returncode == 0 and r.stderr == "", r.stderr
        assert np.array_equal(np.fromfile(tmp_path / "l.bin", dtype="<i4").reshape(H, W), want.labels), clean
        assert np.array_equal(np.fromfile(tmp_path / "u.bin", dtype=np.float64).reshape(H, W), np.where(d, 1.0, -1.0))   # --dump-u is the run's own
        assert np.array_equal(read_pgm(tmp_path / "m.pgm"), want.pieces.astype(np.uint8) * 255), clean
        lab, table = CU.label(want.pieces, 4)
        rows = (tmp_path / "m.csv").read_text().splitlines()[1:]
        assert len(rows) == table.size == want.K and [int(x.split(",")[2]) for x in rows] == [int(a) for a in table["area"]]
        k = int(np.argmax(table["area"]))
        assert r.stdout.splitlines()[-1].split() == ["roi"] + [str(int(table[f][k])) for f in ("x0", "y0", "x1", "y1", "area")], r.stdout
        loops, _ = CT.trace(want.pieces, 4, True)
        assert len((tmp_path / "c.txt").read_text().splitlines()) == loops.size
        objects = [line for line in r.stdout.splitlines() if line.startswith("objects:")]
        assert len(objects) == 1 and f"objects_a={want.K} objects_b={want.K} tp={want.K} fp=0 fn=0" in objects[0], r.stdout
    # without --split the blob is one object; a radius of 0 splits nothing
    r = run(cli, *base, "--split", "0", "--measure", str(tmp_path / "m0.csv"))
    assert r.returncode == 0 and len((tmp_path / "m0.csv").read_text().splitlines()) == 1 + 3
