"""GPU: the device zlib encoder (csrc/deflate.hip, ops.deflate_rows) and the tester's --device-deflate route.  The oracle is
Python's zlib, which is exact: zlib.decompress restores the input bytes and verifies the Adler-32 trailer.  The size conditions
are derived, not measured: every stream is within prv2_deflate_bound (what stored blocks cost), a run of zeros costs under 3
bytes per length-258 match (cap len / 64) and equal 16-bit rows of 193 bytes are matches at distance 193 (cap len / 16) -- zlib
level 1 meets both caps by a wide margin, an encoder that stores everything meets neither.

Files written with device_deflate hold the pixels of the device route's files, not their bytes (another deflate stream)."""
import os
import struct
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
torch.set_grad_enabled(False)


@pytest.fixture(params=["torch"])
def ops(request, monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    monkeypatch.setattr(ops, "DISPATCH", request.param)
    return ops


def _S():
    from patchrefinerv2_amd import lib as L
    return L.load().prv2_deflate_segment()


def _bound(n):
    from patchrefinerv2_amd import lib as L
    return L.load().prv2_deflate_bound(n)


def _streams(ops, frames, length, stride=None):
    """frames: numpy uint8 arrays of at least ``length`` bytes -> the zlib stream of each, checked against zlib"""
    stride = stride or max(16, (length + 15) // 16 * 16)
    host = np.full((len(frames), stride), 0xA5, dtype=np.uint8)  # pad bytes that must not leak into the stream
    for f, a in enumerate(frames):
        host[f, :length] = a[:length]
    out, nb = ops.deflate_rows(torch.from_numpy(host).to(DEV), length)
    out, nb = out.cpu().numpy(), nb.cpu().numpy()
    assert out.shape == (len(frames), _bound(length)) and nb.dtype == np.int64
    res = []
    for f in range(len(frames)):
        assert 0 < nb[f] <= _bound(length), (f, nb[f])
        z = out[f, :nb[f]].tobytes()
        d = zlib.decompressobj()
        got = d.decompress(z) + d.flush()
        assert got == host[f, :length].tobytes(), (f, length)
        assert d.eof and not d.unused_data and zlib.decompress(z) == got
        res.append(z)
    return res


def _contents(n, S):
    """name -> n bytes of every content class the encoder has a separate path for"""
    rng = np.random.Generator(np.random.PCG64(17))
    block = rng.integers(0, 256, 40000, dtype=np.uint8)
    straddle = rng.integers(0, 256, n, dtype=np.uint8)  # the only repeat lies across the first segment boundary
    if n > S + 40:
        straddle[S - 20:S + 20] = straddle[S - 60:S - 20]
    return dict(zeros=np.zeros(n, dtype=np.uint8), random=rng.integers(0, 256, n, dtype=np.uint8),
                period3=np.resize(np.array([7, 200, 31], dtype=np.uint8), n), period4=np.resize(np.array([1, 2, 3, 250], dtype=np.uint8), n),
                far_repeat=np.resize(block, n), straddle=straddle, all_bytes=np.resize(np.arange(256, dtype=np.uint8), n))


LENGTHS = ("0", "1", "2", "3", "257", "258", "259", "S-1", "S", "S+1", "3S+17")


def _length(name, S):
    return int(eval(name.replace("3S", "3*S"), {"S": S}))


@pytest.mark.parametrize("name", LENGTHS)
def test_round_trip_every_content(ops, name):
    S = _S()
    n = _length(name, S)
    c = _contents(max(n, 1), S)
    for kind, a in c.items():
        z = _streams(ops, [a], n)[0]
        if kind == "random":
            assert len(z) <= _bound(n)  # incompressible: the stored fallback
    # three frames of different content in one call, at a stride larger than the length
    _streams(ops, [c["zeros"], c["random"], c["period3"]], n, stride=(n + 15) // 16 * 16 + 48)


def _depth_map(h, w, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    d = 3.0 + 40.0 * x / w + 6.0 * np.sin(y / 9.0) + 12.0 * (x > 0.6 * w) + 0.02 * rs.rand(h, w).astype(np.float32)
    d[h // 3:h // 3 + 5, w // 4:w // 4 + 9] = np.nan
    return d.astype(np.float32)


def _png_scanlines(data):
    """(IHDR fields, inflated IDAT) of a PNG file, every chunk's CRC checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    o, ihdr, idat, tags = 8, None, b"", []
    while o < len(data):
        n, tag = struct.unpack(">I", data[o:o + 4])[0], data[o + 4:o + 8]
        body = data[o + 8:o + 8 + n]
        assert struct.unpack(">I", data[o + 8 + n:o + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        tags.append(tag)
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        if tag == b"IDAT":
            idat += body
        o += 12 + n
    assert tags[0] == b"IHDR" and tags[-1] == b"IEND"
    return ihdr, zlib.decompress(idat)


@pytest.mark.parametrize("shape", [(64, 96), (300, 500)])
def test_real_scanlines_round_trip_and_png(ops, shape):
    from patchrefinerv2_amd import output as O
    h, w = shape
    S = _S()
    d = torch.from_numpy(_depth_map(h, w, h)).to(DEV)
    with np.errstate(invalid="ignore"):
        rows = {2: ops.quantize16_rows(d[None], 256.0), 1: ops.mask_rows((d[None] > 25.0)),
                3: O.colorize_device(torch.nan_to_num(d, nan=-99.0), cmap="Spectral", vminp=0, vmaxp=100)[1]}
    for bpp, r in rows.items():
        n = h * (1 + bpp * w)
        out, nb = ops.deflate_rows(r, n)
        z = out[0, :int(nb[0])].cpu().numpy().tobytes()
        want = r[0, :n].cpu().numpy().tobytes()
        assert zlib.decompress(z) == want and len(z) <= _bound(n)
        if shape == (300, 500):
            assert n > 2 * S  # the file spans several segments
        hd, lines = _png_scanlines(O.png_bytes_from_stream(O.ihdr(w, h, bpp), z))
        assert hd == struct.unpack(">IIBBBBB", O.ihdr(w, h, bpp)) and lines == want
        try:
            import io
            from PIL import Image
        except ImportError:
            continue
        img = np.asarray(Image.open(io.BytesIO(O.png_bytes_from_stream(O.ihdr(w, h, bpp), z))))
        px = np.frombuffer(want, dtype=np.uint8).reshape(h, 1 + bpp * w)[:, 1:]
        assert np.array_equal(img.astype(">u2").view(np.uint8).reshape(h, -1) if bpp == 2 else img.reshape(h, -1), px)


def test_size_conditions(ops):
    n = 1 << 20
    z = _streams(ops, [np.zeros(n, dtype=np.uint8)], n)[0]
    print(f"1 MiB of zeros: {len(z)} bytes (cap {n // 64}, zlib level 1 {len(zlib.compress(bytes(n), 1))})")
    assert len(z) <= n // 64
    rng = np.random.Generator(np.random.PCG64(5))
    row = np.concatenate([[0], rng.integers(0, 65536, 96).astype(">u2").view(np.uint8)]).astype(np.uint8)  # filter byte + 96 16-bit pixels
    img = np.tile(row, 400)
    z = _streams(ops, [img], img.size)[0]
    print(f"400 equal 16-bit rows: {len(z)} bytes of {img.size} (cap {img.size // 16}, zlib level 1 {len(zlib.compress(img.tobytes(), 1))})")
    assert len(z) <= img.size // 16
    m = 200000
    z = _streams(ops, [rng.integers(0, 256, m, dtype=np.uint8)], m)[0]
    assert len(z) <= _bound(m)


def _mixed(S):
    c = _contents(3 * S + 17, S)
    return np.concatenate([c["zeros"][:S // 2], c["random"][:S // 2 + 5], c["period3"][:S], c["all_bytes"][:3 * S + 17]])[:3 * S + 17]


def test_determinism_and_both_dispatch_routes(monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    S = _S()
    a = _mixed(S)
    got = {}
    for route in ("torch", "ctypes", "torch"):
        monkeypatch.setattr(ops, "DISPATCH", route)
        z = _streams(ops, [a, a[::-1].copy()], a.size)
        assert got.setdefault("z", z) == z, route


def test_side_stream_after_producer_event(ops):
    """the output stage's pattern: the producer kernel on one stream, the encoder on another, ordered by an event"""
    d = torch.from_numpy(_depth_map(300, 500, 1)).to(DEV)[None]
    n = 300 * (1 + 2 * 500)
    ref_out, ref_nb = ops.deflate_rows(ops.quantize16_rows(d, 256.0), n)
    ref = ref_out[0, :int(ref_nb[0])].cpu().numpy().tobytes()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        rows = ops.quantize16_rows(d, 256.0)
        ev = torch.cuda.Event()
        ev.record(s1)
    with torch.cuda.stream(s2):
        s2.wait_event(ev)
        out, nb = ops.deflate_rows(rows, n)
        rows.record_stream(s2)
    s2.synchronize()
    assert out[0, :int(nb[0])].cpu().numpy().tobytes() == ref and zlib.decompress(ref) == rows[0, :n].cpu().numpy().tobytes()


# ------------------------------------------------------------------------------------------------------------------ Tester
def _tester(tmp_path, work, device_deflate):
    from patchrefinerv2_amd import models, weights as W  # noqa: F401  (registers the model classes)
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.tester import ImageDataset, RunnerInfo, Tester
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    name = "v1_dav2s_1080p_m1"
    w = WORKLOADS[name]
    if not (tmp_path / "imgs").exists():
        (tmp_path / "imgs").mkdir()
        for i in range(2):
            np.save(str(tmp_path / "imgs" / f"f{i}.npy"), np.random.RandomState(60 + i).rand(90, 160, 3).astype(np.float32))
    m = build_model(model_config(name, prec="bf16x3", max_batch=int(w.get("max_batch", 41)), n_streams=3))
    m.load_state_dict(W.synth_state_dict(state_spec(name), seed=0), strict=True)
    ds = ImageDataset(str(tmp_path / "imgs"), min_depth=1e-3, max_depth=80, image_resolution=w["raw"])
    info = RunnerInfo(save=True, work_dir=str(tmp_path / work), device_output=True, device_deflate=device_deflate, output_workers=4)
    return Tester(None, info, ds, m), w


def _same_pictures(a_dir, b_dir, count):
    names = sorted(os.listdir(a_dir))
    assert names == sorted(os.listdir(b_dir)) and len(names) == count
    for n in names:
        a, b = (_png_scanlines(open(os.path.join(d, n), "rb").read()) for d in (a_dir, b_dir))
        assert a[0] == b[0] and a[1] == b[1], n


def test_tester_device_deflate_writes_the_device_routes_pictures(tmp_path):
    kw = dict(seed=621)
    plain, w = _tester(tmp_path, "dev", False)
    plain.run(cai_mode=w["mode"], image_raw_shape=w["raw"], patch_split_num=w["split"], **kw)
    defl, _ = _tester(tmp_path, "defl", True)
    defl.run(cai_mode=w["mode"], image_raw_shape=w["raw"], patch_split_num=w["split"], **kw)
    _same_pictures(tmp_path / "dev", tmp_path / "defl", 2 * 4)
    assert defl.last_output_stage.device_deflate and defl.last_output_stage.files == plain.last_output_stage.files == 8
    assert 0 < defl.last_output_stage.bytes_d2h < plain.last_output_stage.bytes_d2h
    plain, _ = _tester(tmp_path, "pl_dev", False)
    plain.generate_pl(cai_mode="r4", image_raw_shape=w["raw"], patch_split_num=w["split"], count_thr=0.2, **kw)
    defl, _ = _tester(tmp_path, "pl_defl", True)
    defl.generate_pl(cai_mode="r4", image_raw_shape=w["raw"], patch_split_num=w["split"], count_thr=0.2, **kw)
    _same_pictures(tmp_path / "pl_dev", tmp_path / "pl_defl", 2 * 5)
    assert 0 < defl.last_output_stage.bytes_d2h < plain.last_output_stage.bytes_d2h
