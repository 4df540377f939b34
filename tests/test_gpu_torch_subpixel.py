"""Segmenter.contours(subpixel=True) on the GPU: on device tensors of two shapes and channel counts, on a side stream, loops and points
equal Context.contours_subpixel() of the segmenter's contexts and the restatement; the default contours() is unchanged.  ONE fresh child
process (torch imported first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_subpixel_contours_equal_context_contours_subpixel():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_subpixel_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_subpixel child ok" in out.stdout
