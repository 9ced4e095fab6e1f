#!/usr/bin/env python
"""Pin the shape contracts of the conv entry points: writes tests/golden/conv_contract.json.

Run ONCE against the library whose answers are to be kept (the commit in front of a change of the host-side dispatch): no GPU is
needed, the ``*_supported`` predicates look at the descriptor alone and a refused call returns in front of any launch.  The file
records, per predicate, its answers over an explicit grid of descriptors and over single-field departures from an accepted one
(hex bit strings, first case = most significant bit), and the prv2_last_error() text of the refused calls listed in REFUSALS.
tests/test_conv_contract_host.py builds the same cases from this module and compares.

    python tools/make_conv_contract_golden.py            # PRV2_HIP_LIB=<other build> to record another library
"""
from __future__ import annotations

import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from patchrefinerv2_amd import lib as L  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "conv_contract.json")
PTR = 16  # a 16-byte aligned non-null pointer that is never followed (as in tests/test_cabi.py)

GRID_H, GRID_W = (3, 4, 9), (15, 16, 23, 24, 70)
GRID_CIN, GRID_COUT = (32, 34, 48, 64, 96), (30, 32, 64, 128, 130, 256)
GRID_PREC = (L.PREC_F32, L.PREC_BF16X3, L.PREC_BF16)
PREDICATES = ("ups", "tail", "pre", "ln_gate", "ln_gate_taps", "f6")


def roundup(a, b):
    return (a + b - 1) // b * b


def desc(*shape, **k):
    """shape = (h, w, cin, cout, prec): 3x3 s1 p1, ldx = roundup(cin, 4), ldy = roundup(cout, 4) + 4; keyword arguments overwrite single fields"""
    h, w, cin, cout, prec = shape
    f = dict(n=1, h=h, w=w, cin=cin, cout=cout, kh=3, kw=3, stride=1, pad=1, ldx=roundup(cin, 4), ldy=roundup(cout, 4) + 4, x_bstride=0, y_bstride=0,
             relu_in=0, act=0, convt_k=0, ld_mul=0, ld_res=0, ld_res2=0, prec=prec, force_generic=0, ln_eps=1e-6, part=0, same_pad=0, fmt=0)
    f.update(k)
    return L.ConvDesc(**f)


def ups_src(**k):
    f = dict(x=PTR, h=2, w=8, ld=32, channels=32, bstride=0)
    f.update(k)
    return L.UpsSrc(**f)


# the accepted descriptor the departures start from: (h, w, cin, cout, prec)
BASE = {"ups": (9, 24, 64, 128, L.PREC_BF16X3), "tail": (9, 24, 64, 32, L.PREC_BF16X3), "pre": (9, 24, 64, 32, L.PREC_BF16X3),
        "ln_gate": (9, 24, 64, 128, L.PREC_BF16X3), "ln_gate_taps": (9, 24, 64, 256, L.PREC_BF16X3), "f6": (9, 24, 64, 256, L.PREC_F16F6)}
DEPARTURES = (("kh=1", dict(kh=1)), ("stride=2", dict(stride=2)), ("pad=0", dict(pad=0)), ("convt_k=3", dict(convt_k=3)), ("same_pad", dict(same_pad=1)),
              ("force_generic", dict(force_generic=1)), ("part=1", dict(part=1)), ("relu_in", dict(relu_in=1)), ("fmt=1", dict(fmt=1)), ("ldy=cout", None),
              ("x extent 2^29", dict(h=4096, w=4096, ldx=32)), ("x extent 2^29 - 2^17", dict(h=4095, w=4096, ldx=32)))
UPS_DEPARTURES = (("channels=0", dict(channels=0)), ("channels=16", dict(channels=16, ld=16)), ("channels=32", dict(channels=32)),
                  ("channels=cin", dict(channels=64, ld=64)), ("channels=cin+32", dict(channels=96, ld=96)), ("ld=34", dict(ld=34)), ("h=0", dict(h=0)))


def cases(pred):
    """[(label, ConvDesc, UpsSrc or None)]: the base, the grid, the departures -- in a fixed order"""
    out = [("base", desc(*BASE[pred]), ups_src() if pred == "ups" else None)]
    for prec in GRID_PREC + ((L.PREC_F16F6,) if pred == "f6" else ()):
        for h in GRID_H:
            for w in GRID_W:
                for cin in GRID_CIN:
                    for cout in GRID_COUT:
                        out.append((f"{h}x{w} {cin}->{cout} {L.PREC_LABEL[prec]}", desc(h, w, cin, cout, prec), ups_src() if pred == "ups" else None))
    for label, k in DEPARTURES:
        k = dict(ldy=BASE[pred][3]) if k is None else k
        out.append((label, desc(*BASE[pred], **k), ups_src() if pred == "ups" else None))
    if pred == "ups":
        out += [(label, desc(*BASE[pred]), ups_src(**k)) for label, k in UPS_DEPARTURES]
    return out


def ask(lib, pred, d, u):
    if pred == "ups":
        return lib.prv2_conv2d_ups_supported(C.byref(d), C.byref(u))
    fn = {"tail": lib.prv2_conv2d_tail_supported, "pre": lib.prv2_conv2d_pre_supported, "ln_gate": lib.prv2_conv3x3_ln_gate_supported,
          "ln_gate_taps": lib.prv2_conv3x3_ln_gate_taps_supported, "f6": lib.prv2_conv3x3_f6_supported}[pred]
    return fn(C.byref(d))


def answers(lib, pred):
    bits = [ask(lib, pred, d, u) for _, d, u in cases(pred)]
    assert set(bits) <= {0, 1}, (pred, set(bits))
    return bits


def to_hex(bits):
    pad = bits + [0] * (-len(bits) % 4)
    return "".join(f"{int(''.join(map(str, pad[i:i + 4])), 2):x}" for i in range(0, len(pad), 4))


# refused calls: name -> (predicate that must say 0, entry point, descriptor [, source])
_B3 = L.PREC_BF16X3
REFUSALS = {
    "ups kh=1": ("ups", "conv2d_ups", desc(*BASE["ups"], kh=1)),
    "ups width 23": ("ups", "conv2d_ups", desc(9, 23, 64, 128, _B3)),
    "ups channels=16": ("ups", "conv2d_ups", desc(*BASE["ups"]), dict(channels=16, ld=16)),
    "tail ldy=cout": ("tail", "conv2d_tail", desc(*BASE["tail"], ldy=32)),
    "tail f32": ("tail", "conv2d_tail", desc(9, 24, 64, 32, L.PREC_F32)),
    "pre fmt=1": ("pre", "conv2d_pre", desc(*BASE["pre"], fmt=1)),
    "pre height 3": ("pre", "conv2d_pre", desc(3, 24, 64, 32, _B3)),
    "pre x extent 2^29": ("pre", "conv2d_pre", desc(*BASE["pre"], h=4096, w=4096, ldx=32)),
    "ln_gate 128 width 23": ("ln_gate", "conv3x3_ln_gate", desc(9, 23, 64, 128, _B3)),
    "ln_gate 256 cin 48": ("ln_gate", "conv3x3_ln_gate", desc(9, 24, 48, 256, _B3)),
    "ln_gate 64 channels": ("ln_gate", "conv3x3_ln_gate", desc(9, 24, 64, 64, _B3)),
    "ln_gate_taps width 15": ("ln_gate_taps", "conv3x3_ln_gate_taps", desc(9, 15, 64, 256, _B3)),
    "ln_gate_taps 128 channels": ("ln_gate_taps", "conv3x3_ln_gate_taps", desc(9, 24, 64, 128, _B3)),
    "f6 stride=2": ("f6", "conv3x3_f6", desc(*BASE["f6"], stride=2)),
    "ln_gate_f6 cin 96": ("f6", "conv3x3_ln_gate_f6", desc(9, 24, 96, 256, L.PREC_F16F6)),
}


def refuse(lib, name):
    """-> (the predicate's answer, the call's return value, prv2_last_error()) of REFUSALS[name]; every pointer is the dummy PTR"""
    pred, entry, d, *src = REFUSALS[name]
    u = ups_src(**(src[0] if src else {}))
    taps = L.TapTables()
    dp, P = C.byref(d), PTR
    call = {
        "conv2d_ups": lambda: lib.prv2_conv2d_ups(dp, P, C.byref(u), P, P, P, P, None, P, None),
        "conv2d_tail": lambda: lib.prv2_conv2d_tail(dp, P, P, P, P, P, None, P, P, 4, 4, P, None),
        "conv2d_pre": lambda: lib.prv2_conv2d_pre(dp, P, P, P, P, d.ldy, P, P, None, P, None),
        "conv3x3_ln_gate": lambda: lib.prv2_conv3x3_ln_gate(dp, P, P, P, P, P, P, P, None, None, P, None),
        "conv3x3_ln_gate_taps": lambda: lib.prv2_conv3x3_ln_gate_taps(dp, P, P, P, C.byref(taps), P, P, P, P, None, None, P, None),
        "conv3x3_f6": lambda: lib.prv2_conv3x3_f6(dp, P, P, None, None, 1.0, 1.0, None, P, None),
        "conv3x3_ln_gate_f6": lambda: lib.prv2_conv3x3_ln_gate_f6(dp, P, P, P, None, 0, P, P, P, P, None, None, 1.0, 1.0, None, P, None),
    }[entry]
    yes = ask(lib, pred, d, u)
    if yes:  # a call is only made where the predicate refuses: nothing may reach a launch
        return yes, None, None
    rc = call()
    return yes, rc, lib.prv2_last_error().decode()


def main():
    lib = L.load()
    rec = {"library_abi": L.ABI_VERSION, "answers": {}, "cases": {}, "refusals": {}}
    for pred in PREDICATES:
        bits = answers(lib, pred)
        assert bits[0] == 1, f"{pred}: the base descriptor is not accepted"
        assert sum(bits) >= 20 and len(bits) - sum(bits) >= 20, (pred, sum(bits), len(bits))
        rec["answers"][pred], rec["cases"][pred] = to_hex(bits), len(bits)
        print(f"  {pred}: {sum(bits)} yes / {len(bits) - sum(bits)} no")
    for name in REFUSALS:
        yes, rc, msg = refuse(lib, name)
        assert yes == 0 and rc not in (None, 0) and msg, (name, yes, rc, msg)
        rec["refusals"][name] = msg
        print(f"  {name}: {msg}")
    with open(OUT, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    assert os.path.getsize(OUT) < 64 * 1024
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
