"""chan_vese --colorspace without a GPU: the option is refused together with -g and for an unknown name, each with its message, before any
device is touched; -h lists it."""
import cli_util
from cli_util import BIN as CLI, head_comment


def run(*args):
    return cli_util.run(CLI, *args, timeout=120)


def test_colorspace_is_validated(tmp_path):
    img = tmp_path / "a.ppm"
    with open(img, "wb") as f:
        f.write(b"P6\n40 40\n255\n" + bytes(4800))
    r = run("-i", str(img), "--colorspace", "ycrcb", "-g")
    assert r.returncode == 1 and "--colorspace" in r.stderr and "-g" in r.stderr and "grayscale" in r.stderr
    r = run("-i", str(img), "-g", "--colorspace", "YUV")
    assert r.returncode == 1 and "--colorspace" in r.stderr and "grayscale" in r.stderr
    for bad in ("lab", "rgb", "ycbcr"):
        r = run("-i", str(img), "--colorspace", bad)
        assert r.returncode == 1 and "Invalid colour space requested." in r.stderr and "ycrcb, yuv" in r.stderr
    r = run("-i", str(img), "--colorspace")
    assert r.returncode == 1 and "error: the required argument for option '--colorspace' is missing" in r.stderr


def test_help_lists_colorspace():
    text = run("-h").stdout
    assert "--colorspace arg" in text and "ycrcb | yuv" in text and "not with -g" in text
    assert "--colorspace" in head_comment()
