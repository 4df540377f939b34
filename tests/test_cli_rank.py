"""chan_vese --rank / --rank-radius: without a GPU the options are validated, each refusal with its message, before any device is
touched, and -h lists them; on the GPU (marked) every spelling gives the restatement's planes (--dump-planes) and the mask of the capi
sequence -- set_image, rank_planes_to, the start, run, get_mask --, --init otsu acts on the rank planes, and with --local the rank filter
runs first."""
import numpy as np
import pytest

import local_util as LU
import rank_util as U
import cli_util
from cli_util import BIN as CLI, head_comment, write_pgm


def run(*args):
    return cli_util.run(CLI, *args, timeout=120)


def read_pgm_tail(path, h, w):
    return np.frombuffer(open(path, "rb").read()[-h * w:], dtype=np.uint8).reshape(h, w)


def test_rank_is_validated(tmp_path):
    img = tmp_path / "a.ppm"
    with open(img, "wb") as f:
        f.write(b"P6\n40 40\n255\n" + bytes(4800))
    for bad in ("mean", "copy", "gradient", "3"):
        r = run("-i", str(img), "--rank", bad)
        assert r.returncode == 1 and "Invalid rank filter requested." in r.stderr and "median, min, max, open, close, tophat, bothat" in r.stderr
    for bad in ("-1", "128"):
        r = run("-i", str(img), "--rank", "tophat", "--rank-radius", bad)
        assert r.returncode == 1 and "Rank radius must be between 0 and 127" in r.stderr
    for bad in ("-1", "8", "127"):
        r = run("-i", str(img), "--rank", "median", "--rank-radius", bad)
        assert r.returncode == 1 and "Rank radius must be between 0 and 7 for a median" in r.stderr
    r = run("-i", str(img), "--rank-radius", "3")
    assert r.returncode == 1 and "--rank-radius" in r.stderr and "--rank" in r.stderr
    r = run("-i", str(img), "--rank")
    assert r.returncode == 1 and "error: the required argument for option '--rank' is missing" in r.stderr
    r = run("-i", str(img), "-g", "--rank", "open", "--lambda1", "1", "1", "1")     # a rank filter keeps the channel count
    assert r.returncode == 1 and "Too many lambda1 values for a grayscale image." in r.stderr


def test_help_lists_rank():
    text = run("-h").stdout
    assert "--rank arg" in text and "median | min | max | open | close | tophat | bothat" in text and "--rank-radius arg (=1)" in text
    assert "--rank median|min|max|open|close|tophat|bothat" in head_comment()


@pytest.mark.gpu
def test_cli_rank_gives_the_planes_and_the_mask_of_the_capi_sequence(tmp_path):
    from chan_vese_amd import capi
    n = U.PROP_N
    for name, image, R in [(nm, U.ramp_image, 3) for nm in ("min", "max", "open", "close", "bothat", "MEDIAN")] + \
            [("median", U.salt_image, U.SALT_R), ("tophat", U.ramp_image, U.RAMP_R)]:
        plane = np.array(image())
        img = tmp_path / "prop.pgm"
        write_pgm(img, plane)
        for init in ("checkerboard", "otsu") if name in ("median", "tophat") else ("otsu",):
            out, planes_out = tmp_path / f"{name}_{init}.pgm", tmp_path / f"{name}_{init}_planes.pgm"
            r = run("-i", str(img), "-g", "--rank", name, "--rank-radius", str(R), "--init", init, "-N", "40", "--dump-mask", str(out),
                    "--dump-planes", str(planes_out), "--verbose")
            assert r.returncode == 0, r.stderr
            assert np.array_equal(read_pgm_tail(planes_out, n, n), U.fast(plane, R, U.NAMES[name.lower()])), (name, init)
            with capi.Context(n, n, 1) as src, capi.Context(n, n, 1) as ctx:
                src.set_image([plane])
                src.rank_planes_to(ctx, R, name)
                ctx.init_otsu() if init == "otsu" else ctx.init_checkerboard()     # Otsu acts on the planes the run sees
                steps, _ = ctx.run(40)
                mask = ctx.get_mask()
            assert f"chan_vese: {steps} iterations" in r.stderr, (name, init, r.stderr)
            assert np.array_equal(read_pgm_tail(out, n, n) != 0, mask != 0), (name, init)


@pytest.mark.gpu
def test_cli_rank_runs_in_front_of_local(tmp_path):
    n = U.PROP_N
    plane = np.array(U.salt_image())
    img, planes_out = tmp_path / "salt.pgm", tmp_path / "planes.pgm"
    write_pgm(img, plane)
    r = run("-i", str(img), "-g", "--local", "stack", "--local-radius", "2", "--rank", "median", "--rank-radius", "1", "-N", "5",
            "--dump-planes", str(planes_out))
    assert r.returncode == 0, r.stderr
    want = LU.expected([U.fast(plane, 1, U.MEDIAN)], 3, 2, LU.STACK)
    assert np.array_equal(read_pgm_tail(planes_out, 3 * n, n), np.concatenate(want, axis=0))
