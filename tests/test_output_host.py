"""CPU: the host half of the GPU output stage (patchrefinerv2_amd/output.py).  The percentile restatement equals np.percentile, the
colour table and index rule equal matplotlib, the writer pool's files are byte-identical to write_png16 / write_png8, a worker
error surfaces in flush(), and the new C entry points are declared, bound, exported and reject bad arguments without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prv2_output_workspace_bytes", "prv2_rows_bytes", "prv2_order_stats", "prv2_colorize_rows", "prv2_quantize16_rows",
           "prv2_pl_uncertainty_rows", "prv2_mask_rows", "prv2_upsample_bilinear_map")
OPS = ("order_stats", "colorize_rows", "quantize16_rows", "pl_uncertainty_rows", "mask_rows", "upsample_bilinear_map")
PCTS = (0, 2, 5, 33.3, 50, 95, 99.5, 100)


def test_percentile_restatement_equals_numpy():
    from patchrefinerv2_amd import output as O
    rs = np.random.RandomState(7)
    for n in (1, 2, 3, 7, 64, 1000, 1001, 12345, 99991, 518401):
        for a in (rs.randn(n).astype(np.float32) * 30, rs.rand(n).astype(np.float32), np.round(rs.rand(n) * 4).astype(np.float32)):
            s = np.sort(a)
            for p in PCTS:
                lo, hi, _ = O.percentile_ranks(n, p)
                got, want = O.percentile_from_sorted(s[lo], s[hi], s[-1], n, p), np.percentile(a, p)
                assert got.dtype == want.dtype == np.float32 and got == want, (n, p, got, want)


def test_percentile_restatement_nan_and_inf():
    from patchrefinerv2_amd import output as O
    a = np.array([3.0, np.nan, 1.0, 2.0, 5.0], dtype=np.float32)
    b = np.array([3.0, np.inf, 1.0, -np.inf, 5.0, 2.0], dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for arr in (a, b):
            s = np.sort(arr)
            for p in PCTS:
                lo, hi, _ = O.percentile_ranks(len(arr), p)
                got, want = O.percentile_from_sorted(s[lo], s[hi], s[-1], len(arr), p), np.percentile(arr, p)
                assert (np.isnan(got) and np.isnan(want)) or got == want, (arr, p, got, want)


@pytest.mark.parametrize("cmap", ["Spectral", "magma_r", "gray_r", "jet", "turbo_r"])
def test_lut_and_index_rule_equal_matplotlib(cmap):
    import matplotlib
    from patchrefinerv2_amd import output as O
    lut = O.colormap_lut(cmap)
    n = lut.shape[0] - 3
    assert lut.dtype == np.uint8 and lut.shape == (259, 4)
    rs = np.random.RandomState(3)
    special = [-1.0, -1e-8, -0.0, 0.0, 1e-8, 0.5, 1.0 - 2 ** -24, 1.0, 1.0 + 2 ** -23, 2.0, np.nan, np.inf, -np.inf, 255 / 256, 1 / 256]
    for dt in (np.float32, np.float64):
        x = np.concatenate([np.array(special), rs.rand(20000) * 1.4 - 0.2, np.arange(257) / 256.0]).astype(dt)
        want = matplotlib.colormaps[cmap](x, bytes=True)
        got = lut[O.lut_index(x, n)]
        assert np.array_equal(got, want), int((got != want).sum())


def test_writer_pool_files_equal_write_png(tmp_path):
    from patchrefinerv2_amd import output as O
    from patchrefinerv2_amd.tester import write_png8, write_png16
    rs = np.random.RandomState(5)
    h, w = 37, 53
    u16 = (rs.rand(h, w) * 65535).astype(np.uint16)
    rgb = (rs.rand(h, w, 3) * 255).astype(np.uint8)
    gray = ((rs.rand(h, w) > 0.7) * 255).astype(np.uint8)
    write_png16(str(tmp_path / "a16.png"), u16)
    write_png8(str(tmp_path / "a8.png"), rgb)
    write_png8(str(tmp_path / "ag.png"), gray)

    def rows(arr, bpp):
        raw = np.zeros((h, 1 + bpp * w), dtype=np.uint8)
        raw[:, 1:] = arr.reshape(h, bpp * w)
        return raw.tobytes()

    st = O.OutputStage(str(tmp_path / "out"), workers=64)
    assert st.workers == O.MAX_WORKERS == 16 and O.OutputStage(str(tmp_path / "out")).workers == 8  # capped; default 8
    st.write_rows(str(tmp_path / "out" / "a16.png"), w, h, 2, rows(u16.astype(">u2").view(np.uint8), 2))
    st.write_rows(str(tmp_path / "out" / "a8.png"), w, h, 3, rows(rgb, 3))
    st.write_rows(str(tmp_path / "out" / "ag.png"), w, h, 1, memoryview(rows(gray, 1)))
    st.close()
    for name in ("a16.png", "a8.png", "ag.png"):
        assert (tmp_path / "out" / name).read_bytes() == (tmp_path / name).read_bytes(), name


@pytest.mark.parametrize("kind, depth, ctype", [("gray", 8, 0), ("rgb", 8, 2), ("rgba", 8, 6), ("u16", 16, 0)])
def test_writers_cover_the_colour_type_table(tmp_path, kind, depth, ctype):
    """write_png8 / write_png16 against a container assembled here: signature, IHDR, one IDAT of zlib level 6, IEND"""
    import struct
    import zlib
    from PIL import Image
    from patchrefinerv2_amd.output import write_png8, write_png16
    h, w = 5, 7
    rs = np.random.RandomState(11)
    if kind == "u16":
        arr = rs.randint(0, 65536, (h, w)).astype(np.uint16)
        samples = arr.astype(">u2").tobytes()
    else:
        arr = rs.randint(0, 256, (h, w) + {"gray": (), "rgb": (3,), "rgba": (4,)}[kind]).astype(np.uint8)
        samples = arr.tobytes()
    path = str(tmp_path / f"{kind}.png")
    (write_png16 if kind == "u16" else write_png8)(path, arr)
    stride = len(samples) // h
    rows = b"".join(b"\x00" + samples[y * stride:(y + 1) * stride] for y in range(h))  # filter byte 0 per scanline

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)
    want = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows, 6))
            + chunk(b"IEND", b""))
    with open(path, "rb") as f:
        assert f.read() == want
    back = np.asarray(Image.open(path))
    assert back.shape == arr.shape and np.array_equal(back.astype(arr.dtype), arr)


def test_worker_error_surfaces_in_flush(tmp_path):
    from patchrefinerv2_amd import output as O
    st = O.OutputStage(str(tmp_path), workers=2)
    st.write_rows(str(tmp_path / "no_such_dir" / "x.png"), 2, 2, 1, bytes(6))
    st.write_rows(str(tmp_path / "ok.png"), 2, 2, 1, bytes(6))
    with pytest.raises(OSError):
        st.flush()
    st.flush()  # raised once
    st.close()
    assert (tmp_path / "ok.png").exists()


def test_device_wrappers_reject_host_inputs_and_unbuilt_options():
    from patchrefinerv2_amd import output as O
    with pytest.raises(ValueError, match="host-only"):
        O.colorize_device(torch.zeros(4, 4), gamma_corrected=True)
    with pytest.raises(ValueError, match="host-only"):
        O.colorize_device(torch.zeros(4, 4), value_transform=lambda x: x)
    with pytest.raises(ValueError, match="GPU"):
        O.colorize_device(torch.zeros(4, 4))


def test_tester_rejects_device_output_without_device_map(tmp_path):
    from patchrefinerv2_amd.tester import RunnerInfo, Tester

    class M:
        supports_return_device = False
    t = Tester(None, RunnerInfo(save=True, device_output=True, work_dir=str(tmp_path)), [], M())
    with pytest.raises(ValueError, match="device map"):
        t.run()
    assert Tester(None, RunnerInfo(save=False, device_output=True), [], M()).run() == []  # nothing to save: the default route


def test_entry_points_declared_bound_exported_and_ops_registered():
    from patchrefinerv2_amd import lib as L, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20  # additive: the ABI stays at 20
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.SIGNATURES and hasattr(raw, name), name
    ops = torch_ops.load()
    for name in OPS:
        assert name in torch_ops.OPS
        getattr(ops, name).default._schema
    assert "-> (Tensor, Tensor)" in str(ops.order_stats.default._schema)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.quantize16_rows(torch.zeros(1, 4, 4), 256.0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.mask_rows(torch.zeros(1, 4, 4, dtype=torch.bool))


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    err = lambda: lib.prv2_last_error().decode()  # noqa: E731
    p = ctypes.c_void_p(4096)  # 16-byte aligned, never dereferenced: every call fails its argument check before a launch
    odd = ctypes.c_void_p(4100)
    ranks = (ctypes.c_int64 * 2)(0, -1)
    assert lib.prv2_output_workspace_bytes(0) == -1 and lib.prv2_output_workspace_bytes(2) == 2 * lib.prv2_output_workspace_bytes(1) > 0
    assert lib.prv2_rows_bytes(3, 7, 3) == 80 and lib.prv2_rows_bytes(2160, 3840, 2) == (2160 * 7681 + 15) // 16 * 16
    assert lib.prv2_rows_bytes(0, 7, 3) == -1 and lib.prv2_rows_bytes(3, 7, 5) == -1
    ws = lib.prv2_output_workspace_bytes(1)
    assert lib.prv2_order_stats(None, None, -99.0, None, 0.0, 1, 4, 4, ranks, 2, p, p, p, ws, None) != 0 and "null" in err()
    assert lib.prv2_order_stats(p, None, -99.0, None, 0.0, 1, 4, 4, None, 2, p, p, p, ws, None) != 0 and "null" in err()
    assert lib.prv2_order_stats(p, None, -99.0, None, 0.0, 1, 4, 4, ranks, 9, p, p, p, ws, None) != 0 and "ranks" in err()
    assert lib.prv2_order_stats(p, None, -99.0, None, 0.0, 1, 4, 4, ranks, 2, p, p, None, ws, None) != 0 and "workspace" in err()
    assert lib.prv2_order_stats(p, None, -99.0, None, 0.0, 1, 4, 4, ranks, 2, p, p, p, ws - 1, None) != 0 and "workspace" in err()
    assert lib.prv2_order_stats(p, None, -99.0, None, 0.0, 0, 4, 4, ranks, 2, p, p, p, ws, None) != 0 and "frame count" in err()
    assert lib.prv2_order_stats(p, None, -99.0, None, 0.0, 1, 0, 4, ranks, 2, p, p, p, ws, None) != 0 and "shape" in err()
    assert lib.prv2_order_stats(p, None, -99.0, None, 0.0, 4, 16384, 16384, ranks, 2, p, p, p, 4 * ws, None) != 0 and "exceed" in err()
    rb = lib.prv2_rows_bytes(4, 4, 3)
    assert lib.prv2_colorize_rows(p, None, -99.0, 1, 4, 4, None, p, 256, 0, p, rb, None) != 0 and "null" in err()
    assert lib.prv2_colorize_rows(p, None, -99.0, 1, 4, 4, p, None, 256, 0, p, rb, None) != 0 and "lut" in err()
    assert lib.prv2_colorize_rows(p, None, -99.0, 1, 4, 4, p, p, 0, 0, p, rb, None) != 0 and "colours" in err()
    assert lib.prv2_colorize_rows(p, None, -99.0, 1, 4, 4, p, p, 5000, 0, p, rb, None) != 0 and "colours" in err()
    assert lib.prv2_colorize_rows(p, None, -99.0, 1, 4, 4, p, p, 256, 0, None, rb, None) != 0 and "null" in err()
    assert lib.prv2_colorize_rows(p, None, -99.0, 1, 4, 4, p, p, 256, 0, odd, rb, None) != 0 and "aligned" in err()
    assert lib.prv2_colorize_rows(p, None, -99.0, 1, 4, 4, p, p, 256, 0, p, rb - 16, None) != 0 and "stride" in err()
    assert lib.prv2_colorize_rows(p, None, -99.0, 1, 4, 4, p, p, 256, 0, p, rb + 8, None) != 0 and "stride" in err()
    q = lib.prv2_rows_bytes(4, 4, 2)
    assert lib.prv2_quantize16_rows(None, 1, 4, 4, 256.0, p, q, None) != 0 and "null" in err()
    assert lib.prv2_quantize16_rows(p, 1, 4, 4, 256.0, p, q - 16, None) != 0 and "stride" in err()
    assert lib.prv2_pl_uncertainty_rows(p, None, 1, 4, 4, p, p, 256, p, q, p, rb, None) != 0 and "null" in err()
    assert lib.prv2_pl_uncertainty_rows(p, p, 1, 4, 4, p, p, 256, p, q, p, q, None) != 0 and "stride" in err()
    assert lib.prv2_mask_rows(None, 1, 4, 4, p, 32, None) != 0 and "null" in err()
    assert lib.prv2_mask_rows(p, 1, 4, 4, p, 16, None) != 0 and "stride" in err()
    assert lib.prv2_upsample_bilinear_map(p, 1, 4, 4, None, 8, 8, None) != 0 and "null" in err()
    assert lib.prv2_upsample_bilinear_map(p, 1, 4, 4, p, 0, 8, None) != 0 and "shape" in err()
    with pytest.raises(RuntimeError):
        L.check(lib.prv2_mask_rows(None, 1, 4, 4, p, 32, None), "mask_rows")
