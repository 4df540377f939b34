"""Segmenter(colour=).segment on the GPU: masks, counts, planes and level sets of 3 x 64 x 48 x 3 device tensors equal those of a Segmenter
with colour=None fed the restated planes (colour_util), for both layouts and both spaces; the conversion comes behind Perona-Malik
(images() is forward(the smoothed planes)); levels=2 converts in front of the restricts.  ONE fresh child process (torch imported
first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_colour_equals_the_restated_planes():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_colour_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_colour child ok" in out.stdout
