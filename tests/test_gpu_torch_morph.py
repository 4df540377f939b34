"""Segmenter's morphology on the GPU: clean_masks(morph=...) and Segmenter.morph on device tensors equal the restatement,
segment(init=("mask", t)) equals a Segmenter started from the same level sets, and the levels > 1 refusal is raised.  ONE fresh child
process (torch imported first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_morphology_and_mask_starts():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_morph_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_morph child ok" in out.stdout
