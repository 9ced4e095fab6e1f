"""CPU: the host half of the device deflate route (csrc/deflate.hip entry points, patchrefinerv2_amd/output.py, tools/test.py).  The
entry points are declared, bound and exported on ABI 20, the size bound is what stored blocks cost, every argument rejection of
prv2_deflate_rows happens before a launch, the PNG container around a given zlib stream is the one png_bytes builds, and the
opt-in flags are wired and checked -- all without a GPU."""
import ctypes
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prv2_deflate_segment", "prv2_deflate_bound", "prv2_deflate_workspace_bytes", "prv2_deflate_rows")


def test_entry_points_declared_bound_exported_and_op_registered():
    from patchrefinerv2_amd import lib as L, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20  # additive: the ABI stays at 20
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.SIGNATURES and hasattr(raw, name), name
    assert L.load().prv2_abi_version() == 20
    ops = torch_ops.load()
    assert "deflate_rows" in torch_ops.OPS
    assert "-> (Tensor, Tensor)" in str(ops.deflate_rows.default._schema)
    import torch
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.deflate_rows(torch.zeros(1, 16, dtype=torch.uint8), 16)  # no CPU implementation to fall into


def test_segment_and_bound():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    S = lib.prv2_deflate_segment()
    assert S >= 32768
    assert lib.prv2_deflate_bound(-1) == -1
    for n in (0, 1, S - 1, S, S + 1, 2160 * 7681, 2160 * 11521):
        b = lib.prv2_deflate_bound(n)
        assert b % 16 == 0 and n + 6 <= b <= n + n // 512 + 64, (n, b)
    assert lib.prv2_deflate_workspace_bytes(0, 16) == -1 and lib.prv2_deflate_workspace_bytes(1, -1) == -1
    assert lib.prv2_deflate_workspace_bytes(2, S + 1) == 2 * lib.prv2_deflate_workspace_bytes(1, S + 1) > 2 * S


def test_deflate_rows_rejects_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    err = lambda: lib.prv2_last_error().decode()  # noqa: E731
    p = ctypes.c_void_p(4096)  # 16-byte aligned, never dereferenced: every call fails its argument check before a launch
    odd = ctypes.c_void_p(4100)
    n, length, rs = 2, 1000, 1008
    b, ws = lib.prv2_deflate_bound(length), lib.prv2_deflate_workspace_bytes(2, length)
    call = lib.prv2_deflate_rows
    assert call(None, n, length, rs, p, b, p, p, ws, None) != 0 and "null" in err()
    assert call(p, n, length, rs, None, b, p, p, ws, None) != 0 and "null" in err()
    assert call(p, n, length, rs, p, b, None, p, ws, None) != 0 and "null" in err()
    assert call(p, n, length, rs, p, b, p, None, ws, None) != 0 and "workspace" in err()
    assert call(p, n, length, rs, p, b, p, p, ws - 1, None) != 0 and "workspace" in err()
    assert call(p, 0, length, rs, p, b, p, p, ws, None) != 0 and "frame count" in err()
    assert call(p, n, -1, rs, p, b, p, p, ws, None) != 0 and "length" in err()
    assert call(p, n, length, rs, p, b - 16, p, p, ws, None) != 0 and "stride" in err() and "bound" in err()
    assert call(p, n, length, rs, p, b + 8, p, p, ws, None) != 0 and "stride" in err()
    assert call(p, n, length, rs + 8, p, b, p, p, ws, None) != 0 and "stride" in err()
    assert call(p, n, length, 992, p, b, p, p, ws, None) != 0 and "stride" in err()  # shorter than the length
    assert call(odd, n, length, rs, p, b, p, p, ws, None) != 0 and "aligned" in err()
    assert call(p, n, length, rs, odd, b, p, p, ws, None) != 0 and "aligned" in err()
    assert call(p, n, length, rs, p, b, odd, p, ws, None) != 0 and "aligned" in err()
    assert call(p, n, length, rs, p, b, p, odd, ws, None) != 0 and "aligned" in err()
    with pytest.raises(RuntimeError):
        L.check(call(None, n, length, rs, p, b, p, p, ws, None), "deflate_rows")


def test_png_bytes_from_stream_is_png_bytes_container():
    from patchrefinerv2_amd import output as O
    rs = np.random.RandomState(3)
    for bpp, (h, w) in ((1, (5, 7)), (2, (37, 53)), (3, (16, 9))):
        raw = np.zeros((h, 1 + bpp * w), dtype=np.uint8)
        raw[:, 1:] = rs.randint(0, 256, (h, bpp * w))
        rows, hd = raw.tobytes(), O.ihdr(w, h, bpp)
        z = zlib.compress(rows, 6)
        assert O.png_bytes_from_stream(hd, z) == O.png_bytes(hd, rows)
        assert O.png_bytes_from_stream(hd, memoryview(np.frombuffer(z, dtype=np.uint8))) == O.png_bytes(hd, rows)
        other = O.png_bytes_from_stream(hd, zlib.compress(rows, 1))  # another stream: the payload is taken as given
        assert other != O.png_bytes(hd, rows) and zlib.compress(rows, 1) in other


def test_output_stage_constructs_with_device_deflate(tmp_path):
    from patchrefinerv2_amd import output as O
    st = O.OutputStage(str(tmp_path), workers=64, device_deflate=True)
    assert st.device_deflate and st.workers == O.MAX_WORKERS == 16 and st.stream is None and st.bytes_d2h == 0
    st.write_rows(str(tmp_path / "a.png"), 2, 2, 1, bytes(6))  # host rows still go through the pool
    st.close()
    assert (tmp_path / "a.png").read_bytes() == O.png_bytes(O.ihdr(2, 2, 1), bytes(6))
    assert not O.OutputStage(str(tmp_path)).device_deflate and O.OutputStage(str(tmp_path)).workers == 8


def test_tester_and_cli_reject_device_deflate_without_device_output(tmp_path):
    from patchrefinerv2_amd.tester import RunnerInfo, Tester

    class M:
        supports_return_device = True
    t = Tester(None, RunnerInfo(save=True, device_deflate=True, work_dir=str(tmp_path)), [], M())
    with pytest.raises(ValueError, match="device_output"):
        t.run()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "no_such_config.py", "--save", "--device-deflate"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--device-deflate needs --device-output" in r.stderr, r.stderr[-2000:]
