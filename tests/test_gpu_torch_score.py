"""Segmenter.score() on the GPU: on device tensors of two shapes the integers equal Context.score() on the same data and the restatement,
and bool and uint8 truth tensors agree.  ONE fresh child process (torch imported first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_score_equals_context_score():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_score_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_score child ok" in out.stdout
