"""bin/chan_vese --morph / --morph-radius / --init-mask: -h lists them and bad arguments exit non-zero with a message before any device is
touched (CPU); on the GPU `--morph open --morph-radius 2 --dump-mask` is the restatement (morph_util.py) of the `--dump-mask` without it --
with and without cleaning flags, and --roi, --measure and --contours speak of the same morphed mask --, and `--init-mask` with `-N 0` dumps
the mask it was given."""
import numpy as np
import pytest

import components_util as CU
import contour_util as CT
import morph_util as M
from chan_vese_amd import synth
from cli_util import cli, head_comment, read_pnm as read_pgm, run

H, W = 40, 56


def write_pnm(path, img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P5" if img.ndim == 2 else b"P6", img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def test_help_lists_the_morph_flags(cli):
    text = run(cli, "-h").stdout
    assert "--morph arg" in text and "--morph-radius arg (=1)" in text and "--init-mask arg" in text and "dilate | erode | open | close" in text
    head = head_comment()
    assert "--morph" in head and "--morph-radius" in head and "--init-mask" in head


def test_morph_flags_are_validated(cli, tmp_path):
    write_pnm(tmp_path / "a.pgm", np.zeros((H, W), dtype=np.uint8))
    write_pnm(tmp_path / "small.pgm", np.zeros((H, W - 1), dtype=np.uint8))
    write_pnm(tmp_path / "colour.ppm", np.zeros((H, W, 3), dtype=np.uint8))
    base = ["-i", str(tmp_path / "a.pgm"), "-g"]
    for args, text in (
            (["--morph", "thin"], "Invalid morphology requested.\nCorrect values are: dilate, erode, open, close."),
            (["--morph-radius", "2"], "A radius (--morph-radius) needs an operation (--morph)."),
            (["--morph", "open", "--morph-radius", "-1"], "Morphology radius must be a finite number >= 0."),
            (["--morph", "open", "--morph-radius", "nan"], "Morphology radius must be a finite number >= 0."),
            (["--morph"], "error: the required argument for option '--morph' is missing"),
            (["--init-mask"], "error: the required argument for option '--init-mask' is missing"),
            (["--init-mask", str(tmp_path / "missing.pgm")], "missing.pgm\" does not exists!"),
            (["--init-mask", str(tmp_path / "small.pgm")], f"is {W - 1} x {H}, the input {W} x {H}: they must have the same size."),
            (["--init-mask", str(tmp_path / "colour.ppm")], "(a mask start must be a binary PGM)!"),
            (["--init-mask", str(tmp_path / "a.pgm"), "--levels", "2"], "A mask start (--init-mask) cannot be combined with a coarse-to-fine run (--levels)"),
            (["--init-mask", str(tmp_path / "a.pgm"), "--rect", "1,1,5,5"], "Cannot initialize with both --rect and --init-mask"),
            (["--init-mask", str(tmp_path / "a.pgm"), "--init", "otsu"], "Cannot initialize with both --init otsu and --init-mask")):
        r = run(cli, *base, *args)
        assert r.returncode == 1 and text in r.stderr, (args, r.returncode, r.stderr)


@pytest.mark.gpu
def test_morph_applies_to_what_the_mask_outputs_write(cli, tmp_path):
    img = synth.disk(H, 200, 50, noise=60, seed=4, h=H, w=W)
    write_pnm(tmp_path / "a.pgm", img)
    base = ["-i", str(tmp_path / "a.pgm"), "-g", "-t", "0", "-N", "12"]
    for clean, kw in (([], {}), (["--min-area", "4", "--fill-holes", "3"], dict(min_area=4, fill_holes=3)), (["-I"], {})):
        plain = run(cli, *base, *clean, "--dump-mask", str(tmp_path / "m0.pgm"), "--dump-u", str(tmp_path / "u0.bin"))
        assert plain.returncode == 0, plain.stderr
        m0 = read_pgm(tmp_path / "m0.pgm")
        assert set(np.unique(m0)) <= {0, 255} and 0 < (m0 != 0).sum() < H * W
        u0 = np.fromfile(tmp_path / "u0.bin", dtype=np.float64).reshape(H, W)
        assert np.array_equal(m0 != 0, CU.clean(M.mask_of(u0, "-I" in clean), 4, kw.get("min_area", 0), kw.get("fill_holes", 0), False) != 0)
        for op, radius in (("open", "2"), ("close", "1.5"), ("dilate", "1"), ("erode", "0")):
            r = run(cli, *base, *clean, "--morph", op, "--morph-radius", radius, "--dump-mask", str(tmp_path / "m1.pgm"), "--dump-u", str(tmp_path / "u1.bin"),
                    "--roi", "--measure", str(tmp_path / "m.csv"), "--contours", str(tmp_path / "c.txt"))
            assert r.returncode == 0 and r.stderr == "", r.stderr
            assert (tmp_path / "u0.bin").read_bytes() == (tmp_path / "u1.bin").read_bytes()        # --dump-u is the run's own level set
            want = M.morph(m0 != 0, M.OPS[["none", "dilate", "erode", "open", "close"].index(op)], int(float(radius) ** 2))
            assert np.array_equal(read_pgm(tmp_path / "m1.pgm"), want.astype(np.uint8) * 255), (clean, op, radius)
            # --roi, --measure and --contours speak of the same mask
            lab, table = CU.label(want, 4)
            rows = (tmp_path / "m.csv").read_text().splitlines()[1:]
            assert len(rows) == table.size and [int(x.split(",")[2]) for x in rows] == [int(a) for a in table["area"]]
            if table.size:
                k = int(np.argmax(table["area"]))
                assert r.stdout.split() == ["roi"] + [str(int(table[f][k])) for f in ("x0", "y0", "x1", "y1", "area")], r.stdout
            else:
                assert r.stdout.strip() == "roi none"
            loops, _ = CT.trace(want, 4, True)
            assert len((tmp_path / "c.txt").read_text().splitlines()) == loops.size
    # the default radius is 1: the 4-neighbour cross
    r = run(cli, *base, "--morph", "dilate", "--dump-mask", str(tmp_path / "m2.pgm"))
    plain = run(cli, *base, "--dump-mask", str(tmp_path / "m0.pgm"))
    assert r.returncode == 0 and np.array_equal(read_pgm(tmp_path / "m2.pgm") != 0, M.dilate(read_pgm(tmp_path / "m0.pgm") != 0, 1))


@pytest.mark.gpu
def test_init_mask_round_trips_with_no_iterations(cli, tmp_path):
    img = synth.disk(H, 200, 50, noise=20, seed=4, h=H, w=W)
    write_pnm(tmp_path / "a.pgm", img)
    rng = np.random.default_rng(3)
    mask = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), size=(H, W))
    mask.reshape(-1)[:4] = [0, 1, 2, 255]
    write_pnm(tmp_path / "start.pgm", mask)
    for extra in ([], ["-S"]):                                               # (Perona-Malik smooths the planes, not the start)
        r = run(cli, "-i", str(tmp_path / "a.pgm"), "-g", "-N", "0", "--init-mask", str(tmp_path / "start.pgm"), *extra,
                "--dump-mask", str(tmp_path / "out.pgm"), "--dump-u", str(tmp_path / "u.bin"))
        assert r.returncode == 0 and r.stderr == "", r.stderr
        assert np.array_equal(read_pgm(tmp_path / "out.pgm"), (mask != 0).astype(np.uint8) * 255)
        assert np.array_equal(np.fromfile(tmp_path / "u.bin", dtype=np.float64).reshape(H, W), np.where(mask != 0, 1.0, -1.0))
    # and the run iterates from it
    r = run(cli, "-i", str(tmp_path / "a.pgm"), "-g", "-t", "0", "-N", "10", "--init-mask", str(tmp_path / "start.pgm"), "--verbose", "--dump-mask", str(tmp_path / "o2.pgm"))
    assert r.returncode == 0 and "10 iterations" in r.stderr, r.stderr
