"""Segmenter(localized=R) and Segmenter(phases=4) on the GPU, now through the batch calls: three small members give the masks / labels of
capi single runs of the same inputs.  ONE fresh child process (torch imported first; a failed child fails the test), as the torch tests
of the two flows."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenters_equal_the_capi_single_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_march_batch_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_march_batch child ok" in out.stdout
