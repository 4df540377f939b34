"""cvh_localized_run_batch / cvh_multiphase_run_batch without a card: both names are exported with the header's argument counts, and the
Python-side argument errors of capi.localized_run_batch / capi.multiphase_run_batch are raised before the library is entered (the
stand-in members below have no handle: reaching the library would fail on them first)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cvh_localized_run_batch", "cvh_multiphase_run_batch")


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build()
    from chan_vese_amd import capi as m
    return m


class NoHandle:
    """a member that only Python looks at"""
    channels = 1


@pytest.mark.parametrize("name", NAMES)
def test_exported_with_the_headers_argument_count(capi, name):
    hdr = open(os.path.join(ROOT, "include", "chanvese_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = re.findall(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr)
    assert len(found) == 1, found
    declared = [a.strip() for a in found[0].split(",")]
    assert len(declared) == 9
    assert name in capi.EXPORTS
    fn = getattr(capi.lib(), name)
    assert len(fn.argtypes) == len(declared)


def test_localized_run_batch_argument_errors(capi):
    members = [NoHandle(), NoHandle(), NoHandle()]
    for call, text in [
        (lambda: capi.localized_run_batch([], 3, 2), "no members"),
        (lambda: capi.localized_run_batch(iter(()), [3], 2), "no members"),
        (lambda: capi.localized_run_batch(members, [3, 3], 2), "2 values for 3 members"),
        (lambda: capi.localized_run_batch(members, [3, 3, 3, 3], 2), "4 values for 3 members"),
        (lambda: capi.localized_run_batch(members, [], 2), "0 values for 3 members"),
        (lambda: capi.localized_run_batch(members, 3, -1, trace=True), "trace=True needs max_steps >= 0"),
    ]:
        with pytest.raises(ValueError, match=text):
            call()


def test_multiphase_run_batch_argument_errors(capi):
    a, b = NoHandle(), NoHandle()
    for call, text in [
        (lambda: capi.multiphase_run_batch([], 2), "no pairs"),
        (lambda: capi.multiphase_run_batch(iter(()), 2), "no pairs"),
        (lambda: capi.multiphase_run_batch([(a, b), (a,)], 2), "every member is a pair"),
        (lambda: capi.multiphase_run_batch([(a, b, a)], 2), "every member is a pair"),
        (lambda: capi.multiphase_run_batch([(a, b)], -1, trace=True), "trace=True needs max_steps >= 0"),
    ]:
        with pytest.raises(ValueError, match=text):
            call()
