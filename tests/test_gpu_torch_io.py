"""chan_vese_amd.torch_io on the GPU: Segmenter.segment on 16 synthetic disks given as (N, H, W), (N, 3, H, W) and (N, H, W, 3) uint8 device
tensors, with and without Perona-Malik, with a tensor as initial level set: masks byte for byte those of the host-buffer pipeline; a torch
operation enqueued right behind segment on the current stream sees the final masks; a source written on a busy side stream is read complete.
Each form runs in ONE fresh child process (torch imported first, one child at a time; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("form", ["gray", "planar3", "inter3"])
def test_segmenter_equals_the_host_buffer_pipeline(form):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_io_child.py"), form],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert f"torch_io child ok: {form}" in out.stdout
