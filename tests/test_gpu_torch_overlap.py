"""Segmenter.overlaps() / .match() on the GPU: on three members of mixed content, on a side stream, the rows equal Context.overlaps() of the
segmenter's contexts and the restatement; frame to frame, the components of frame 1 are the labels of frame 2 and every object matches at
1/2.  ONE fresh child process (torch imported first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_overlaps_and_frame_to_frame_match():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_overlap_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_overlap child ok" in out.stdout
