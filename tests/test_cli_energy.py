"""bin/chan_vese --energy / --energy-every: the flags are validated before any device is touched and -h lists them (CPU); on the GPU the
printed lines parse, hold %.17g numbers that are capi's Context.energy() for the same run bit for bit, and a run without the flags
prints what it printed before them -- nothing on stdout -- and leaves the same level set."""
import numpy as np
import pytest

from chan_vese_amd import synth
from cli_util import cli, head_comment, run, write_pgm, write_ppm

H, W = 40, 56


def parse(line, channels, with_iteration):
    """'[iteration ]energy total length area fit_in.. fit_out..' -> (iteration or None, [floats])"""
    tok = line.split()
    it = int(tok.pop(0)) if with_iteration else None
    assert tok[0] == "energy" and len(tok) == 4 + 2 * channels, line
    return it, [float(t) for t in tok[1:]]


def test_energy_flags_are_validated(cli, tmp_path):
    img = tmp_path / "a.pgm"
    write_pgm(img, np.zeros((H, W), dtype=np.uint8))
    r = run(cli, "-i", str(img), "-g", "--energy-every", "-3")
    assert r.returncode == 1 and "Energy interval cannot be negative: -3." in r.stderr
    r = run(cli, "-i", str(img), "-g", "--energy-every")
    assert r.returncode == 1 and "error: the required argument for option '--energy-every' is missing" in r.stderr
    r = run(cli, "-i", str(img), "-g", "--energy-every", "x")
    assert r.returncode == 1 and "error: the argument ('x') for option '--energy-every' is invalid" in r.stderr
    r = run(cli, "-i", str(img), "-g", "--energy=1")
    assert r.returncode == 1 and "error: option '--energy' does not take any arguments" in r.stderr
    for other, word in ((["-V"], "video output (-V)"), (["--reinit", "8"], "reinitialisation (--reinit)"), (["--levels", "2"], "a coarse-to-fine run (--levels)")):
        r = run(cli, "-i", str(img), "-g", "--energy-every", "4", *other)
        assert r.returncode == 1 and "An energy series (--energy-every) cannot be combined with " + word in r.stderr, r.stderr


def test_help_lists_the_energy_flags(cli):
    text = run(cli, "-h").stdout
    assert "--energy  " in text and "--energy-every arg (=0)" in text and "fit_in... fit_out..." in text
    head = head_comment()
    assert "--energy" in head and "--energy-every" in head


@pytest.mark.gpu
def test_energy_lines_match_capi(cli, tmp_path):
    from chan_vese_amd import capi
    img = synth.disk(H, 200, 50, noise=20, seed=4, h=H, w=W)
    write_pgm(tmp_path / "a.pgm", img)
    base = ["-i", str(tmp_path / "a.pgm"), "-g", "-t", "0"]
    # without the flags: nothing on stdout, as before them; with --energy: the same level set and one line more
    plain = run(cli, *base, "-N", "24", "--dump-u", str(tmp_path / "u0.bin"))
    assert plain.returncode == 0 and plain.stdout == "" and plain.stderr == "", (plain.stdout, plain.stderr)
    r = run(cli, *base, "-N", "24", "--energy", "--dump-u", str(tmp_path / "u1.bin"))
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert (tmp_path / "u0.bin").read_bytes() == (tmp_path / "u1.bin").read_bytes()
    lines = r.stdout.splitlines()
    assert len(lines) == 1
    _, final = parse(lines[0], 1, False)
    with capi.Context(H, W, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([img])
        ctx.init_checkerboard()
        assert ctx.run(24)[0] == 24
        e = ctx.energy()
        assert final == [e.total, e.length, e.area, *e.fit_in, *e.fit_out]      # %.17g round-trips a double
        assert np.array_equal(np.fromfile(tmp_path / "u1.bin", dtype=np.float64), ctx.get_levelset().ravel())
    # --energy-every 8 over 20 iterations: lines at 8, 16, 20, then --energy's line for the same level set
    r = run(cli, *base, "-N", "20", "--energy-every", "8", "--energy")
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 4
    rows = [parse(l, 1, True) for l in lines[:3]]
    assert [it for it, _ in rows] == [8, 16, 20]
    assert parse(lines[3], 1, False)[1] == rows[-1][1]
    with capi.Context(H, W, 1, capi.make_params(tol=0.0)) as ctx:
        ctx.set_image([img])
        ctx.init_checkerboard()
        steps, _, series = capi.run_monitored(ctx, max_steps=20, every=8)
    assert steps == 20 and [s for s, _ in series] == [8, 16, 20]
    for (_, vals), (_, e) in zip(rows, series):
        assert vals == [e.total, e.length, e.area, *e.fit_in, *e.fit_out]
    # three channels: three fit_in and three fit_out
    rgb = np.stack([synth.disk(H, 60 + 60 * k, 200 - 50 * k, noise=10, seed=9 + k, h=H, w=W) for k in range(3)], axis=2)
    write_ppm(tmp_path / "c.ppm", rgb)
    r = run(cli, "-i", str(tmp_path / "c.ppm"), "-t", "0", "-N", "6", "--lambda1", "1", "0.8", "0.5", "--nu", "0.01", "--energy")
    assert r.returncode == 0, r.stderr
    _, vals = parse(r.stdout.splitlines()[0], 3, False)
    with capi.Context(H, W, 3, capi.make_params(tol=0.0, nu=0.01, lambda1=[1, 0.8, 0.5])) as ctx:
        ctx.set_image([rgb[:, :, 2], rgb[:, :, 1], rgb[:, :, 0]])     # the loader's planes are B, G, R
        ctx.init_checkerboard()
        assert ctx.run(6)[0] == 6
        e = ctx.energy()
    assert vals == [e.total, e.length, e.area, *e.fit_in, *e.fit_out]
