"""Segmenter(levels=3).segment on the GPU: masks, level sets and per-level counts of 3 x 64 x 144 equal capi.run_coarse_to_fine_batch on
contexts of the same options, for the checkerboard, Otsu (with and without Perona-Malik), disk and rect starts; levels=1 returns the bytes
of the plain path.  ONE fresh child process (torch imported first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_levels_equal_the_capi_driver():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_pyramid_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_pyramid child ok" in out.stdout
