"""Build check on the shipped binary: the gfx950 wide-store data hazard (tools/isa_store_hazard.py).

A >64-bit vector-memory store followed IMMEDIATELY by a VALU write of one of its data registers stores wrong values in
lanes 12-15 of every row of 16 under memory back-pressure (measured: tools/store_hazard_probe.hip); hipcc pads that
only for stores without a register soffset, and the wave kernels use one.  The kernels avoid it by construction (the
stored registers stay live to the end of the 4-row group); this test disassembles every code object of
libchanvese_hip.so and fails if any instantiation has a VALU writer in the issue slot right behind a wide store."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "chan_vese_amd", "csrc", "libchanvese_hip.so")
TOOL = os.path.join(ROOT, "tools", "isa_store_hazard.py")


@pytest.fixture(scope="module")
def report():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} is missing: run __graft_entry__.build() first")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    out = subprocess.run([sys.executable, TOOL, LIB, "--json"], capture_output=True, text=True, timeout=300)
    assert out.returncode in (0, 1), out.stderr[-2000:]
    return json.loads(out.stdout)


def test_no_valu_write_in_the_issue_slot_behind_a_wide_store(report):
    assert report["violations"] == [], report["violations"]


# (wide stores, of them with a register soffset) per 2-pixel CSV instantiation <C, FAST, MINW, POL, ST32>, as the gfx950 build has them
WIDE_STORES = {"ILi1ELb0ELi2ELi1ELb0EEEv": (10, 8),
               "ILi1ELb1ELi3ELi0ELb0EEEv": (18, 16), "ILi1ELb1ELi3ELi1ELb0EEEv": (18, 16), "ILi1ELb1ELi3ELi2ELb0EEEv": (18, 16),
               "ILi3ELb1ELi3ELi0ELb0EEEv": (25, 16), "ILi3ELb1ELi3ELi1ELb0EEEv": (25, 16),
               "ILi1ELb1ELi3ELi0ELb1EEEv": (2, 0), "ILi1ELb1ELi3ELi1ELb1EEEv": (2, 0),
               "ILi3ELb1ELi3ELi0ELb1EEEv": (9, 0), "ILi3ELb1ELi3ELi1ELb1EEEv": (9, 0)}


def test_every_streaming_kernel_with_wide_stores_was_seen(report):
    """The check is only worth something if it saw the kernels it is about: the 2-pixel CSV kernels (16-byte level-set
    stores: >= 8 per instantiation, one per row of the loop bodies), both the context's own entry point (csv_wave2_kernel)
    and the fused batch's (csv_wave2_batch_kernel, the same body: the same stores)."""
    names = {k["kernel"]: k for k in report["kernels"]}
    # (the FP32-state instantiations, last template argument true = "Lb1E", store 8 bytes per lane: outside the hazard)
    own = {n[n.index("ILi"):n.index("EEEv") + 4]: k for n, k in names.items() if "csv_wave2_kernel" in n}
    batch = {n[n.index("ILi"):n.index("EEEv") + 4]: k for n, k in names.items() if "csv_wave2_batch_kernel" in n}
    wave2 = [k for t, k in own.items() if t.endswith("ELb0EEEv")]
    # FP64 state: 1-channel STRICT, three cache policies; 3-channel two cache policies.  FP32 state: 1 and 3 channels, two cache policies each
    assert len(wave2) == 6, sorted(names)
    assert len([t for t in own if t.endswith("ELb1EEEv")]) == 4, sorted(names)
    assert sorted(own) == sorted(WIDE_STORES) and sorted(batch) == sorted(own), (sorted(batch), sorted(own))   # each with its batch entry point
    for k in wave2 + [batch[t] for t in own if t.endswith("ELb0EEEv")]:
        assert k["wide_stores"] >= 8, k
        assert k["register_soffset_stores"] >= 8, k                  # the form hipcc does not pad
        assert k["min_wait_states_register_soffset"].get("valu", 1 << 30) >= 6, k     # by construction: live to the end of the group
    for t in own:   # the batch entry point stores what the context's own kernel stores (tools/isa_store_hazard.py --json on the built library)
        assert (own[t]["wide_stores"], own[t]["register_soffset_stores"]) == WIDE_STORES[t], (t, own[t])
        assert (batch[t]["wide_stores"], batch[t]["register_soffset_stores"]) == WIDE_STORES[t], (t, batch[t])
    # (the 2-pixel Perona-Malik kernel, the other kernel with 16-byte stores, was pruned in round 4: tools/experiments/pruned_flavours/)
