"""Host-side fences of the gather folded into the 256-column gate kernels (no GPU): the entry points' mirrors, and the ISA of the two files whose
kernels run the coarse-tap walk -- built as the Makefile builds them they hold no packed fp32 instruction and no function call."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "patchrefinerv2_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_entry_points_are_mirrored():
    from patchrefinerv2_amd import lib as L, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    for name in ("prv2_conv3x3_ln_gate_taps_supported", "prv2_conv3x3_ln_gate_taps", "prv2_conv3x3_ln_gate_f6_taps"):
        assert re.search(r"\b%s\(" % name, hdr) and name in L.SIGNATURES
    assert {"conv3x3_ln_gate_taps", "conv3x3_ln_gate_f6_taps"} <= set(torch_ops.OPS)
    # prv2_tap_tables: three pointers, five int32, three floats -- the same fields in the same order
    m = re.search(r"typedef struct prv2_tap_tables \{(.*?)\} prv2_tap_tables;", hdr, re.S)
    fields = re.findall(r"(\w+)\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [f for f, _ in L.TapTables._fields_], fields
    assert C.sizeof(L.TapTables) == 56  # (24 + 20 + 12: no padding)


def _makefile_flags(stem):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*=\s*(.*)$", mk, re.M))
    flags = var.get("FLAGS_" + stem, "")
    return re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), flags).split()


@pytest.mark.parametrize("fn", ["conv3x3_gate.hip", "conv3x3_f6.hip"])
def test_gate_files_hold_no_packed_fp32_and_no_call(fn):
    """the walk in the gate kernels' epilogue must stay scalar fp32 (BUILD NOTE in coarse_taps.hip); the per-file flag that does it must not turn the
    runtime's helpers into calls (what a whole-file function attribute did)"""
    import isa_hazard_scan as scan
    flags = _makefile_flags(fn[:-4])
    assert "-packed-fp32-ops" in flags, flags
    counts = scan.packed_fp32_by_kernel(os.path.join(CSRC, fn), defines=flags)
    kernels = {k: v for k, v in counts.items() if "kernel" in k}
    assert any("c256_gate" in k for k in kernels) and all(v == 0 for v in counts.values()), {k: v for k, v in counts.items() if v}
    # no device function survived as a function: everything is inlined into the kernels
    assert all("kernel" in k for k in counts), [k for k in counts if "kernel" not in k]
