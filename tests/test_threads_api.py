"""include/chanvese_hip.h, Threading: cvh_last_error(NULL) is per host thread.  The scenario runs in a fresh child process
(tests/threads_child.py) whose eight threads, released by one barrier, are refused by cvh_create over and over, each with an argument
of its own; the child asserts nothing, every comparison is here.  A child that times out, aborts or dies of a signal fails the test
with its output; nothing is retried.  The calls are refused before the library looks for a device, so this needs no GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import threads_child as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "threads_child.py")
CHILD_TIMEOUT = 600
ERR_ARG = 1   # cvh_status


def run_child(scenario, tmp_path):
    """One child, one scenario: [{name: array}] per thread.  Any end but a clean one is a finding: the test fails with the child's output."""
    cmd = [sys.executable, CHILD, scenario, str(tmp_path)]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"threads child {scenario} still ran after {CHILD_TIMEOUT} s\nstdout: {str(e.stdout)[-3000:]}\nstderr: {str(e.stderr)[-3000:]}")
    assert out.returncode == 0, (scenario, out.returncode, out.stdout[-3000:], out.stderr[-4000:])
    line = json.loads(out.stdout.strip().splitlines()[-1])
    print(f"{scenario}: {line['threads']} threads, {line['seconds']} s in the child")
    failed = {i: e for i, e in enumerate(line["errors"]) if e}
    assert not failed, failed
    data = np.load(os.path.join(str(tmp_path), scenario + ".npz"))
    per_thread = [{} for _ in range(line["threads"])]
    for key in data.files:
        t, name = key[1:].split("_", 1)
        per_thread[int(t)][name] = data[key]
    return per_thread


def test_contextless_errors_are_per_thread(tmp_path):
    """Eight threads, 200 refused cvh_create each, thread k with channels = 10 + k: every cvh_last_error(NULL) read right after a failure
    is a whole message of that family -- never torn text -- and the calling thread's own.  (With one process-wide buffer a thread read
    its neighbour's message: seen on the first run of this test against the library as it was.)"""
    threads = run_child("errors", tmp_path)
    assert len(threads) == TC.ERROR_THREADS == 8
    for k, got in enumerate(threads):
        msgs = str(got["messages"]).split("\n")
        assert len(msgs) == TC.ERROR_CALLS == 200 and (got["codes"] == ERR_ARG).all()
        own = f"cvh_create: channels must be 1 (grayscale) or 3 (colour), got {10 + k}"
        foreign = sorted(set(m for m in msgs if m != own))
        assert not foreign, (k, foreign[:5])


def test_contextless_error_text_survives_other_threads_calls():
    """One process, two threads in turn: a failure on a second thread does not replace what the first thread reads, and a thread that never
    failed reads "no error"."""
    import ctypes
    import threading
    from chan_vese_amd import capi
    L = capi.lib()
    h = ctypes.c_void_p(None)
    assert L.cvh_create(ctypes.byref(h), 16, 16, 7, None, 0) == ERR_ARG
    mine = L.cvh_last_error(None).decode()
    assert mine.endswith("got 7")
    seen = {}

    def other():
        seen["fresh"] = L.cvh_last_error(None).decode()
        g = ctypes.c_void_p(None)
        seen["code"] = L.cvh_create(ctypes.byref(g), 16, 16, 9, None, 0)
        seen["own"] = L.cvh_last_error(None).decode()
        seen["batch_code"] = L.cvh_convert_colour_batch(None, 1, 1, 0, 0)      # the batch calls' context-less text is the same buffer
        seen["batch"] = L.cvh_last_error(None).decode()

    t = threading.Thread(target=other)
    t.start()
    t.join(60)
    assert not t.is_alive()
    assert seen["fresh"] == "no error" and seen["code"] == ERR_ARG and seen["own"].endswith("got 9")
    assert seen["batch_code"] == ERR_ARG and "cvh_convert_colour_batch" in seen["batch"]
    assert L.cvh_last_error(None).decode() == mine
