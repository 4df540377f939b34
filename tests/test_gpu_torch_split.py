"""Segmenter's object split on the GPU: Segmenter.split on device tensors equals the restatement, and after Segmenter.split_levelset
components and measure see the split objects.  ONE fresh child process (torch imported first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_split():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_split_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_split child ok" in out.stdout
