"""Segmenter(rank=).segment on the GPU: masks, counts, planes and level sets of 3 x 64 x 48 device tensors equal those of the capi
sequence (set_image, rank_planes_to, start, run, get_mask) and of a Segmenter with rank=None fed the restated planes (rank_util), for
the median, the top-hat, per-channel closings and a triple of codes; with local= as well the rank filter runs first; the rank planes
come behind Perona-Malik (images() is the filter of the smoothed planes).  ONE fresh child process (torch imported first; a failed child
fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_rank_equals_the_capi_sequence():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_window_child.py"), "rank"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_rank child ok" in out.stdout
