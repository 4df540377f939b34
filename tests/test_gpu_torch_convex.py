"""Segmenter(convex=...) on the GPU: two 64 x 64 device tensors, masks, level sets and relaxed functions equal to the capi path bit for
bit, plain and with edge=K; the refusals.  ONE fresh child process (torch imported first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_convex_equals_the_capi_path():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_convex_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_convex child ok" in out.stdout
