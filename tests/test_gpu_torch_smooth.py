"""Segmenter(smooth=) and Segmenter(edge=, edge_sigma=) on the GPU: planes, edge planes, masks, counts and level sets of 2 x 64 x 64 device
tensors equal the restatements (smooth_util, geodesic_util) and the capi sequences; the stages run rank -> smooth -> local.  ONE fresh
child process (torch imported first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_smooth_and_edge_sigma_equal_the_capi_sequences():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_smooth_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_smooth child ok" in out.stdout
