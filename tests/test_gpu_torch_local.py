"""Segmenter(local=).segment on the GPU: masks, counts, planes and level sets of 3 x 64 x 48 device tensors equal those of the capi
sequence (set_image, local_planes_to, start, run, get_mask) and of a Segmenter with local=None fed the restated planes (local_util), for
the deviation plane, the stack and per-channel statistics; the local planes come behind Perona-Malik (images() is the statistics of the
smoothed planes); levels=2 takes them in front of the restricts.  ONE fresh child process (torch imported first; a failed child fails
the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_local_equals_the_capi_sequence():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_window_child.py"), "local"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_local child ok" in out.stdout
