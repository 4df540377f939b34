"""Segmenter(phases=4) on the GPU: two 64 x 64 device tensors, labels equal to mask_A + 2 mask_B and to the capi path byte for byte; the
post-processing methods take phase = 0 | 1.  ONE fresh child process (torch imported first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_four_phases_equals_the_capi_path():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_multiphase_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_multiphase child ok" in out.stdout
