"""Shared by the tests/test_cli*.py files: where bin/chan_vese is, the fixture that builds it, one way to run it, and the small
PGM / PPM writers and readers those tests use."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin", "chan_vese")
MAIN_CPP = os.path.join(ROOT, "chan_vese_amd", "host", "main.cpp")


@pytest.fixture(scope="module")
def cli():
    import __graft_entry__ as g
    g.build()
    assert os.path.exists(BIN)
    return BIN


def run(cli, *args, timeout=600):
    return subprocess.run([cli, *args], capture_output=True, text=True, timeout=timeout)


def head_comment():
    """main.cpp up to its first #include: the comment at the top of the file."""
    return open(MAIN_CPP).read().split("#include")[0]


def write_pgm(path, img, maxval=255):
    """A binary PGM; above 255 two bytes per sample, most significant first."""
    with open(path, "wb") as f:
        f.write(b"P5\n# synthetic\n%d %d\n%d\n" % (img.shape[1], img.shape[0], maxval))
        f.write(np.ascontiguousarray(img, dtype=np.uint8 if maxval <= 255 else ">u2").tobytes())


def write_ppm(path, rgb):
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(np.ascontiguousarray(rgb, dtype=np.uint8).tobytes())


def read_pnm(path):
    """A binary PGM as (h, w), a binary PPM as (h, w, 3)."""
    data = open(path, "rb").read()
    magic, dims, _, body = data.split(b"\n", 3)
    w, h = map(int, dims.split())
    return np.frombuffer(body, dtype=np.uint8).reshape(h, w, 1 if magic == b"P5" else 3).squeeze()
