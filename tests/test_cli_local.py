"""chan_vese --local / --local-radius: without a GPU the options are validated, each refusal with its message, before any device is
touched, and -h lists them; on the GPU (marked) the flags give the planes and the mask of the capi sequence -- set_image,
local_planes_to, the start, run, get_mask -- for the deviation plane of the proposition's image and for the stack with three lambdas."""
import numpy as np
import pytest

import local_util as U
import cli_util
from cli_util import BIN as CLI, head_comment, write_pgm


def run(*args):
    return cli_util.run(CLI, *args, timeout=120)


def read_pgm_tail(path, h, w):
    return np.frombuffer(open(path, "rb").read()[-h * w:], dtype=np.uint8).reshape(h, w)


def test_local_is_validated(tmp_path):
    img = tmp_path / "a.ppm"
    with open(img, "wb") as f:
        f.write(b"P6\n40 40\n255\n" + bytes(4800))
    r = run("-i", str(img), "--local", "stack")
    assert r.returncode == 1 and "--local stack" in r.stderr and "-g" in r.stderr and "grayscale" in r.stderr
    for bad in ("var", "median", "copy"):
        r = run("-i", str(img), "--local", bad)
        assert r.returncode == 1 and "Invalid local statistic requested." in r.stderr and "mean, dev, stack" in r.stderr
    for bad in ("-1", "128"):
        r = run("-i", str(img), "--local", "dev", "--local-radius", bad)
        assert r.returncode == 1 and "Local radius must be between 0 and 127" in r.stderr
    r = run("-i", str(img), "--local-radius", "3")
    assert r.returncode == 1 and "--local-radius" in r.stderr and "--local" in r.stderr
    r = run("-i", str(img), "--local")
    assert r.returncode == 1 and "error: the required argument for option '--local' is missing" in r.stderr
    # the stack is a three-plane run: one lambda is refused as for a coloured image, -g alone keeps the grey rule
    r = run("-i", str(img), "-g", "--local", "stack", "--lambda1", "1")
    assert r.returncode == 1 and "Number of lambda1 values must be 3" in r.stderr
    r = run("-i", str(img), "-g", "--local", "dev", "--lambda1", "1", "1", "1")
    assert r.returncode == 1 and "Too many lambda1 values for a grayscale image." in r.stderr


def test_help_lists_local():
    text = run("-h").stdout
    assert "--local arg" in text and "mean | dev | stack" in text and "--local-radius arg (=2)" in text and "--dump-planes arg" in text
    assert "--local mean|dev|stack" in head_comment()


@pytest.mark.gpu
def test_cli_local_gives_the_planes_and_the_mask_of_the_capi_sequence(tmp_path):
    from chan_vese_amd import capi
    n = U.PROP_N
    plane = np.array(U.proposition_image())
    img = tmp_path / "prop.pgm"
    write_pgm(img, plane)
    lam = ["0.25", "1", "1"]
    for name, cd, extra, params in (("dev", 1, [], capi.make_params()),
                                    ("stack", 3, ["--lambda1", *lam, "--lambda2", *lam], capi.make_params(lambda1=[0.25, 1, 1], lambda2=[0.25, 1, 1]))):
        for init in ("checkerboard", "otsu"):
            out, planes_out = tmp_path / f"{name}_{init}.pgm", tmp_path / f"{name}_{init}_planes.pgm"
            r = run("-i", str(img), "-g", "--local", name, "--local-radius", "2", "--init", init, "-N", "60", "--dump-mask", str(out),
                    "--dump-planes", str(planes_out), "--verbose", *extra)
            assert r.returncode == 0, r.stderr
            want = U.expected([plane], cd, 2, capi.local_what_codes(name))
            assert np.array_equal(read_pgm_tail(planes_out, cd * n, n), np.concatenate(want, axis=0)), (name, init)
            with capi.Context(n, n, 1) as src, capi.Context(n, n, cd, params) as ctx:
                src.set_image([plane])
                src.local_planes_to(ctx, 2, name)
                ctx.init_otsu() if init == "otsu" else ctx.init_checkerboard()
                steps, _ = ctx.run(60)
                mask = ctx.get_mask()
            assert f"chan_vese: {steps} iterations" in r.stderr, (name, init, r.stderr)
            assert np.array_equal(read_pgm_tail(out, n, n) != 0, mask != 0), (name, init)
