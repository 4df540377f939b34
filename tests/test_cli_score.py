"""bin/chan_vese --truth / --score-tol: -h lists them and a truth of another size is refused before any device is touched (CPU); on the
GPU the printed integers are the restatement's (score_util.py) for the level set the run leaves, and the figures are capi.Score's."""
import math

import numpy as np
import pytest

import score_util as S
from chan_vese_amd import synth
from cli_util import cli, head_comment, run, write_pgm

H, W = 40, 56


def parse(line):
    """'score: iou=.. dice=.. hausdorff=.. assd=.. surface_dice=.. tp=.. fp=.. fn=.. tn=..' -> dict"""
    tok = line.split()
    assert tok[0] == "score:" and [t.split("=")[0] for t in tok[1:]] == ["iou", "dice", "hausdorff", "assd", "surface_dice", "tp", "fp", "fn", "tn"], line
    return {k: (int(v) if k in ("tp", "fp", "fn", "tn") else float(v)) for k, v in (t.split("=") for t in tok[1:])}


def test_help_lists_the_score_flags(cli):
    text = run(cli, "-h").stdout
    assert "--truth arg" in text and "--score-tol arg (=2)" in text and "surface_dice=" in text
    head = head_comment()
    assert "--truth" in head and "--score-tol" in head


def test_score_flags_are_validated(cli, tmp_path):
    write_pgm(tmp_path / "a.pgm", np.zeros((H, W), dtype=np.uint8))
    write_pgm(tmp_path / "small.pgm", np.zeros((H, W - 1), dtype=np.uint8))
    base = ["-i", str(tmp_path / "a.pgm"), "-g"]
    r = run(cli, *base, "--truth", str(tmp_path / "small.pgm"))
    assert r.returncode == 1 and f"is {W - 1} x {H}, the input {W} x {H}: they must have the same size." in r.stderr, r.stderr
    r = run(cli, *base, "--truth", str(tmp_path / "missing.pgm"))
    assert r.returncode == 1 and "missing.pgm" in r.stderr
    r = run(cli, *base, "--score-tol", "3")
    assert r.returncode == 1 and "A score tolerance (--score-tol) needs a ground truth (--truth)." in r.stderr
    r = run(cli, *base, "--truth", str(tmp_path / "a.pgm"), "--score-tol", "-1")
    assert r.returncode == 1 and "Score tolerance must be a finite number >= 0." in r.stderr
    r = run(cli, *base, "--truth")
    assert r.returncode == 1 and "error: the required argument for option '--truth' is missing" in r.stderr


@pytest.mark.gpu
def test_score_line_matches_the_restatement(cli, tmp_path):
    from chan_vese_amd import capi
    img = synth.disk(H, 200, 50, noise=20, seed=4, h=H, w=W)
    truth = S.disk(H, W, H // 2 + 1, W // 2 - 2, H // 4).astype(np.uint8) * 200
    write_pgm(tmp_path / "a.pgm", img)
    write_pgm(tmp_path / "t.pgm", truth)
    base = ["-i", str(tmp_path / "a.pgm"), "-g", "-t", "0", "-N", "24"]
    plain = run(cli, *base, "--dump-u", str(tmp_path / "u0.bin"))
    assert plain.returncode == 0 and plain.stdout == "", (plain.stdout, plain.stderr)
    for extra, tol in (([], 2.0), (["--score-tol", "1.5"], 1.5)):
        r = run(cli, *base, "--truth", str(tmp_path / "t.pgm"), *extra, "--dump-u", str(tmp_path / "u1.bin"))
        assert r.returncode == 0 and r.stderr == "", r.stderr
        assert (tmp_path / "u0.bin").read_bytes() == (tmp_path / "u1.bin").read_bytes()          # the score only reads
        lines = r.stdout.splitlines()
        assert len(lines) == 1
        got = parse(lines[0])
        u = np.fromfile(tmp_path / "u1.bin", dtype=np.float64).reshape(H, W)
        want = S.score(S.mask_of(u), truth != 0, capi.score_tol2(tol))
        assert {k: got[k] for k in ("tp", "fp", "fn", "tn")} == {k: want[k] for k in ("tp", "fp", "fn", "tn")}
        ref = capi.Score(**want)
        for k in ("iou", "dice", "hausdorff", "assd", "surface_dice"):
            assert got[k] == getattr(ref, k) or (math.isnan(got[k]) and math.isnan(getattr(ref, k))), (k, got[k], getattr(ref, k))
        assert want["defined"] == 1 and want["tp"] > 0
