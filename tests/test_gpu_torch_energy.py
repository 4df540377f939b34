"""Segmenter.energies() and Segmenter.segment(energy_every=K) on the GPU: the terms of the last segment()'s contexts equal Context.energy()
for the same inputs bit for bit, the stored series is run_batch_monitored's, and the masks are a plain segment()'s.  ONE fresh child
process (torch imported first; a failed child fails the test)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_segmenter_energies_equal_context_energy():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "torch_energy_child.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "torch_energy child ok" in out.stdout
