"""bin/chan_vese --localized R: the option is validated before any device is touched and -h lists it (CPU); on the GPU the mask and
the level set are the C ABI's for the same start, and a run without --localized writes what it wrote before the option existed."""
import numpy as np
import pytest

import localized_util as L
from cli_util import cli, head_comment, run, write_pgm

H, W = 40, 56


def test_refused_combinations_exit_with_their_message(cli, tmp_path):
    img = tmp_path / "a.pgm"
    write_pgm(img, np.zeros((H, W), dtype=np.uint8))
    base = ["-i", str(img), "-g", "--localized", "5"]
    for other, word in ((["--phases", "4"], "four phases (--phases 4)"), (["--levels", "2"], "a coarse-to-fine run (--levels)"),
                        (["--energy"], "an energy line (--energy)"), (["--energy-every", "4"], "an energy series (--energy-every)"),
                        (["--reinit", "8"], "reinitialisation (--reinit)"), (["-V"], "video output (-V)"),
                        (["--state", "32"], "FP32 state (--state 32)")):
        r = run(cli, *base, *other)
        assert r.returncode == 1 and "Localised regions (--localized) cannot be combined with " + word + "." in r.stderr, (other, r.stderr)
    for bad in ("0", "128", "-2"):
        r = run(cli, "-i", str(img), "-g", "--localized", bad)
        assert r.returncode == 1 and f"Window radius (--localized) must be between 1 and 127: {bad}." in r.stderr, r.stderr


def test_help_lists_the_option(cli):
    text = run(cli, "-h").stdout
    assert "--localized arg" in text
    head = head_comment()
    assert "--localized" in head


@pytest.mark.gpu
def test_mask_and_levelset_are_the_capi_path(cli, tmp_path):
    from chan_vese_amd import capi
    img = L.scene(H, W, 1)[0][0]
    write_pgm(tmp_path / "a.pgm", img)
    base = ["-i", str(tmp_path / "a.pgm"), "-g", "-t", "0", "-N", "10", "--mu", "20"]
    p = capi.make_params(tol=0.0, mu=20.0)

    def capi_run(start):
        with capi.Context(H, W, 1, p) as ctx:
            ctx.set_image([img])
            start(ctx)
            assert capi.localized_run(ctx, 5, 10)[0] == 10
            return ctx.get_levelset(), ctx.get_mask()

    for name, extra, start in (("rect", ["--rect", "10,8,30,20"], lambda c: c.init_rect(10, 8, 30, 20, 1.0, 0.0)),
                               ("otsu", ["--init", "otsu"], lambda c: c.init_otsu())):
        r = run(cli, *base, "--localized", "5", *extra, "--dump-u", str(tmp_path / f"u_{name}.bin"), "--dump-mask", str(tmp_path / f"m_{name}.pgm"))
        assert r.returncode == 0 and r.stdout == "", (r.stdout, r.stderr)
        u, m = capi_run(start)
        assert (tmp_path / f"u_{name}.bin").read_bytes() == u.tobytes()
        pgm = (tmp_path / f"m_{name}.pgm").read_bytes()                        # (--dump-mask writes a binary PGM, 255 where the mask is set)
        assert pgm.startswith(b"P5") and pgm[-H * W:] == (m * 255).astype(np.uint8).tobytes()
    # without --localized: the two-phase run's level set, capi's for the same run bit for bit
    plain = run(cli, *base, "--dump-u", str(tmp_path / "u0.bin"))
    assert plain.returncode == 0 and plain.stdout == "" and plain.stderr == ""
    with capi.Context(H, W, 1, p) as ctx:
        ctx.set_image([img])
        ctx.init_checkerboard()
        assert ctx.run(10)[0] == 10
        assert (tmp_path / "u0.bin").read_bytes() == ctx.get_levelset().tobytes()
