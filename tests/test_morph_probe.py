"""tools/morph_probe.py on the CPU: it imports without a device, refuses bad arguments, and its scipy path -- the one it sets beside the
device's bytes and asserts equal -- is the restatement (morph_util.py) for the probe's operations and radii."""
import os
import subprocess
import sys

import numpy as np
import pytest

import morph_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "morph_probe.py")


@pytest.fixture(scope="module")
def probe():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import morph_probe
    finally:
        sys.path.pop(0)
    return morph_probe


def test_arguments(probe):
    a = probe.parse_args([])
    assert a.sizes == [1024, 2048, 4096] and a.r2 == [2, 25, 400] and (a.reps, a.warmup) == (20, 3) and a.iterations == 50
    for bad in (["--r2", "-1"], ["--reps", "0"], ["--sizes", "8"], ["--cpu-reps", "0"], ["--r2", "x"]):
        r = subprocess.run([sys.executable, TOOL, *bad], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "error" in r.stderr, (bad, r.stderr)
    assert subprocess.run([sys.executable, TOOL, "-h"], capture_output=True, text=True, timeout=120).returncode == 0


def test_the_scipy_path_is_the_restatement(probe):
    pytest.importorskip("scipy.ndimage")
    f = M.noisy_disk(70, 90)
    for op, code in (("open", M.OPEN), ("close", M.CLOSE)):
        for r2 in (2, 25, 400):
            assert np.array_equal(probe.scipy_morph(f, op, r2), M.morph(f, code, r2)), (op, r2)
    with pytest.raises(ValueError):
        probe.scipy_morph(f, "thin", 2)
    assert np.array_equal(probe.disk_structure(25), M.disk_structure(25))


def test_timing_loop_keeps_the_restore_outside(probe):
    calls = []
    probe.per_call(lambda: calls.append("f"), 4, 2, between=lambda: calls.append("b"))
    assert calls == ["b", "f"] * 6
