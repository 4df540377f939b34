"""tests/cpp/test_march_layout.cpp: class sorting, the one lay-out routine (one grid and two) and the loop over the classes present of
chan_vese_amd/csrc/march_flow.h, over synthetic records on the host -- no device is opened."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_march_layout_program():
    exe = os.path.join(ROOT, "bin", "test_march_layout")
    assert os.path.exists(exe), "bin/test_march_layout is built by build() (chan_vese_amd/host/Makefile)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "march lay-out ok", (r.returncode, r.stdout, r.stderr)
