"""bin/chan_vese with the device-side starts: --rect (now cvh_init_rect) against a host-filled run of the same rectangle, --init otsu,
--threshold and --disk against the restated starts (init_util), with and without -S.  The runs need a GPU."""
import subprocess

import numpy as np
import pytest

from chan_vese_amd import synth

import init_util as U
from cli_util import cli, write_pgm, write_ppm

H, W = 40, 56


def dump_u(cli, tmp_path, image, *args):
    out = tmp_path / "u.bin"
    r = subprocess.run([cli, "-i", str(image), *args, "--dump-u", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return np.fromfile(out, dtype=np.float64).reshape(H, W)


@pytest.mark.gpu
def test_rect_is_unchanged(cli, tmp_path):
    """--rect x,y,w,h: ones on exact zeros (src/InteractiveDataRect.cpp:24-25), clipped; and the run from it is the run from a host-filled
    level set of the same rectangle, bit for bit"""
    from chan_vese_amd import capi
    img = synth.disk(H, 200, 50, noise=6, seed=2, h=H, w=W)
    write_pgm(tmp_path / "a.pgm", img)
    for (x, y, rw, rh) in [(10, 8, 30, 20), (-4, 30, 12, 40), (50, -2, 20, 9), (0, 0, W, H), (70, 70, 3, 3)]:
        u0 = dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "--rect", f"{x},{y},{rw},{rh}", "-N", "0")
        want = np.zeros((H, W))
        want[max(y, 0):max(min(y + rh, H), 0), max(x, 0):max(min(x + rw, W), 0)] = 1
        assert np.array_equal(U.bits(u0), U.bits(want))
        assert np.array_equal(U.bits(u0), U.bits(U.start_rect(H, W, x, y, rw, rh, 1.0, 0.0)))
    u8 = dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "--rect", "10,8,30,20", "-N", "8", "-t", "0")
    host = np.zeros((H, W))
    host[8:28, 10:40] = 1
    with capi.Context(H, W, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([img])
        ctx.set_levelset(host)
        assert ctx.run(8)[0] == 8
        assert np.array_equal(U.bits(u8), U.bits(ctx.get_levelset()))
    for bad in ("1,1,0,4", "1,1,4,-2", "1,1,4"):
        r = subprocess.run([cli, "-i", str(tmp_path / "a.pgm"), "-g", "--rect", bad], capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and "You must specify the contour with non-zero dimensions" in r.stderr


@pytest.mark.gpu
def test_otsu_threshold_and_disk_starts(cli, oracle, tmp_path):
    img = synth.disk(H, 200, 50, noise=20, seed=4, h=H, w=W)
    write_pgm(tmp_path / "a.pgm", img)
    t = U.otsu(U.histogram([img]))
    u0 = dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "--init", "otsu", "-N", "0")
    assert np.array_equal(U.bits(u0), U.bits(U.start_threshold([img], t, 1.0, -1.0)))
    assert np.array_equal(U.bits(dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "--threshold", str(t), "-N", "0")), U.bits(u0))
    u0 = dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "--threshold", "0", "-N", "0")
    assert np.array_equal(U.bits(u0), U.bits(U.start_threshold([img], 0, 1.0, -1.0)))
    u0 = dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "--disk", "28,20,12", "-N", "0")
    assert np.array_equal(U.bits(u0), U.bits(U.start_disk(H, W, 28, 20, 12, 1.0, 0.0)))
    u0 = dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "--disk", "-3,50,0", "-N", "0")
    assert not u0.any()
    cb = dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "--init", "checkerboard", "-N", "0")
    assert np.array_equal(U.bits(cb), U.bits(dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "-N", "0")))
    assert np.array_equal(U.bits(cb), U.bits(oracle.checkerboard(H, W)))
    # colour: the grey value is the sum of the three channels
    rgb = np.stack([synth.disk(H, 60 + 60 * k, 200 - 50 * k, noise=10, seed=9 + k, h=H, w=W) for k in range(3)], axis=2)
    write_ppm(tmp_path / "c.ppm", rgb)
    planes = [rgb[:, :, k] for k in range(3)]
    t3 = U.otsu(U.histogram(planes))
    u0 = dump_u(cli, tmp_path, tmp_path / "c.ppm", "--init", "otsu", "-N", "0")
    assert np.array_equal(U.bits(u0), U.bits(U.start_threshold(planes, t3, 1.0, -1.0)))
    u0 = dump_u(cli, tmp_path, tmp_path / "c.ppm", "--threshold", "765", "-N", "0")
    assert (u0 == -1.0).all()
    # with -S the start is taken from the smoothed image
    sm = oracle.perona_malik([img], 30, 0.25, 2)
    u0 = dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "-S", "-K", "30", "-L", "0.25", "-T", "2", "--init", "otsu", "-N", "0")
    assert np.array_equal(U.bits(u0), U.bits(U.start_threshold(sm, U.otsu(U.histogram(sm)), 1.0, -1.0)))
    # and a run from the Otsu start is the oracle's run from the restated start
    u8 = dump_u(cli, tmp_path, tmp_path / "a.pgm", "-g", "--init", "otsu", "-N", "8", "-t", "0")
    u_c, _, _, _ = oracle.csv_run([img], U.start_threshold([img], t, 1.0, -1.0), oracle.make_params(tol=0), 8)
    assert np.abs(u8 - u_c).max() / np.abs(u_c).max() <= 1e-6
