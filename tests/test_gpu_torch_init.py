"""Segmenter.segment(init=...) with the device-side starts on the GPU: "otsu" and each tuple form on 4 x 64 x 144 equal the capi sequence
member by member, and Segmenter.thresholds equals the restated Otsu.  ONE fresh child process (torch imported first; a failed child fails
the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_starts_equal_the_capi_sequence():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_init_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_init child ok" in out.stdout
