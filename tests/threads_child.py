"""Child process of test_threads_api.py: one scenario per fresh process, driven from several host threads at once.

    python threads_child.py <scenario> <out_dir>

The library is loaded in the main thread (capi.lib(): the dlopen and the ctypes signatures) and NOTHING of it is called before the threads
start; ctypes releases the GIL around every call, so the threads do overlap inside the library.  Every thread waits on one barrier, so
that the first library calls of all of them coincide; each thread catches its own exceptions and fills its own slot.  The main thread
joins with a time limit (a thread still alive: their names are printed, exit status 3), writes <out_dir>/<scenario>.npz (arrays
"t<thread>_<name>") and prints one JSON line.  Nothing is asserted here: every comparison is the parent's.

Scenarios:
  errors   eight threads, ERROR_CALLS refused cvh_create each -- thread k with channels = 10 + k, so the message names the thread -- and
           cvh_last_error(NULL) read right after each failure.  Refused before the library looks for a device: launches nothing, and
           runs with or without a GPU."""
import faulthandler
import json
import os
import sys
import threading
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

JOIN_SECONDS = 240
ERROR_THREADS = 8
ERROR_CALLS = 200


def error_job(capi, k, barrier):
    import ctypes as C
    L = capi.lib()
    msgs, codes = [], []
    barrier.wait()
    for _ in range(ERROR_CALLS):
        h = C.c_void_p(None)
        codes.append(L.cvh_create(C.byref(h), 16, 16, 10 + k, None, 0))
        msgs.append(L.cvh_last_error(None).decode("latin-1"))
        if h.value:
            L.cvh_destroy(h)
    return dict(codes=np.array(codes, dtype=np.int64), messages="\n".join(msgs))


def jobs_of(scenario):
    """[(name, callable(capi, barrier))] of a scenario"""
    if scenario == "errors":
        return [(f"errors{k}", lambda capi, b, k=k: error_job(capi, k, b)) for k in range(ERROR_THREADS)]
    raise ValueError(scenario)


def main():
    faulthandler.enable()                        # a fatal signal leaves every thread's Python stack on stderr, which the parent reports
    scenario, out_dir = sys.argv[1], sys.argv[2]
    from chan_vese_amd import capi
    capi.lib()                                   # dlopen + signatures, in the main thread; no cvh_* call before the threads start
    jobs = jobs_of(scenario)
    assert len(jobs) <= 8
    barrier = threading.Barrier(len(jobs))
    results, errors = [None] * len(jobs), [None] * len(jobs)

    def work(slot, fn):
        try:
            results[slot] = fn(capi, barrier)
        except BaseException:                    # the thread's own slot; a broken barrier releases the others
            errors[slot] = traceback.format_exc()
            barrier.abort()

    threads = [threading.Thread(target=work, args=(i, fn), name=name, daemon=True) for i, (name, fn) in enumerate(jobs)]
    t0 = time.time()
    for t in threads:
        t.start()
    deadline = t0 + JOIN_SECONDS
    for t in threads:
        t.join(max(0.0, deadline - time.time()))
    alive = [t.name for t in threads if t.is_alive()]
    if alive:
        print(f"threads still alive after {JOIN_SECONDS} s: {alive}", flush=True)
        os._exit(3)
    arrays = {}
    for i, res in enumerate(results):
        for k, v in (res or {}).items():
            arrays[f"t{i}_{k}"] = np.asarray(v)
    np.savez(os.path.join(out_dir, scenario + ".npz"), **arrays)
    print(json.dumps(dict(scenario=scenario, threads=len(jobs), seconds=round(time.time() - t0, 3), errors=errors)), flush=True)


if __name__ == "__main__":
    main()
