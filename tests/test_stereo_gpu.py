"""GPU: the stereo export (csrc/stereo.hip through ops.stereo_source / ops.stereo_rows, OutputStage.submit_geometry(stereo=...)).  The
oracle is the host specification of patchrefinerv2_amd/output.py (numpy float32): the int32 source maps and the scanline bytes are
compared for equality, on both dispatch routes.  One workgroup of 256 lanes owns a row: lane t has the columns t, t + 256, ...; the
rows of at most 4096 columns and the wider ones are two instances of the kernel."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32 = np.float32
INF = float("inf")
LAYOUTS = ("right", "sbs", "anaglyph")
SHAPES = [(1, 1, 1), (1, 1, 2), (1, 3, 7), (1, 5, 64), (1, 4, 65), (1, 6, 257), (1, 3, 1031), (2, 7, 83)]  # frames, rows, columns
torch.set_grad_enabled(False)


@pytest.fixture(params=["torch", "ctypes"])
def ops(request, monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    monkeypatch.setattr(ops, "DISPATCH", request.param)
    return ops


def _camera(h, w):
    from patchrefinerv2_amd.output import camera_intrinsics
    return camera_intrinsics((h, w), (h, w), fov=63.0) + F32(0.37)


def _image(hi, wi, seed):
    img = np.random.RandomState(100 + seed).rand(3, hi, wi).astype(F32) * F32(1.2) - F32(0.1)  # below 0 and above 1 clamp
    img.reshape(-1)[::31] = np.nan
    return img


def _tie_row(w):
    """the tie case of the issue at the start of a row (k = 50, convergence 1, edge_thr 0.05), then a plane"""
    row = np.full((w,), 1.0, dtype=F32)
    if w >= 2:
        row[1] = 1.04
    return row


# scene name -> (depth [B, h, w], the keyword arguments of the call but the intrinsics)
def _scene(name, B, h, w):
    rs = np.random.RandomState(B * 1000 + h * 31 + w)
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    fx = float(_camera(h, w)[0])
    kw = dict(baseline=0.0, convergence=INF, depth_range=(0.0, INF), edge_thr=0.05)
    if name == "steps":  # blocks in front of a far wall: occlusions and hole runs on their right
        d = np.full((h, w), 6.0, dtype=F32)
        d[:, w // 6:w // 3] = 2.0
        d[h // 2:, w // 2:(3 * w) // 4] = 1.0
        kw.update(baseline=0.03 * w / fx * 6.0)  # the wall moves by about 3 % of the width
    elif name == "slant":  # a plane that stretches in the new view: spans of several columns
        d = (1.0 + 4.0 * (w - x) / w + 0.05 * y).astype(F32)
        kw.update(baseline=0.25 * w / fx, edge_thr=0.5)
    elif name == "random":  # random depth, 10 % invalid pixels of every kind
        d = (1.0 + 5.0 * rs.rand(h, w)).astype(F32)
        idx = rs.choice(h * w, size=(h * w + 9) // 10, replace=False)
        d.reshape(-1)[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.0, -1.5, 0.2, 9.0], dtype=F32), idx.size)
        kw.update(baseline=0.1 * w / fx, depth_range=(0.5, 7.0), edge_thr=0.3)
    elif name == "tie":  # every row starts with the tie case; then the first row all invalid
        d = np.tile(_tie_row(w), (h, 1))
        if h > 1:
            d[0] = np.nan
        kw.update(baseline=50.0 / fx, convergence=1.0)
    elif name == "negative":  # a finite convergence in front of most of the scene: negative disparities, targets off the right edge
        d = (2.0 + 3.0 * rs.rand(h, w) * (x > w // 2) + 0.01 * x).astype(F32)
        kw.update(baseline=0.2 * w / fx, convergence=1.5, edge_thr=0.0)
    else:
        raise KeyError(name)
    d = np.stack([d] + [np.roll(d, 3 * f, axis=1) + F32(0.25 * f) for f in range(1, B)])
    return np.ascontiguousarray(d, dtype=F32), kw


SCENES = ("steps", "slant", "random", "tie", "negative")
_HOST = {}


def _host(name, shape):
    """the specification's maps of a scene, computed once and shared (never modified)"""
    from patchrefinerv2_amd.output import stereo_source_host
    key = (name, shape)
    if key not in _HOST:
        d, kw = _scene(name, *shape)
        k = _camera(*shape[1:])
        maps = [stereo_source_host(d[f], k, **kw) for f in range(shape[0])]
        _HOST[key] = (d, k, kw, np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps]))
    return _HOST[key]


def _rows_to_image(rows, h, wout):
    """scanline buffer [B, bytes] (a device tensor) -> uint8 [B, h, wout, 3]; every filter byte and the tail are zero"""
    r = rows.cpu().numpy()
    body = r[:, :h * (1 + 3 * wout)].reshape(r.shape[0], h, 1 + 3 * wout)
    assert not body[:, :, 0].any() and not r[:, h * (1 + 3 * wout):].any()
    assert r.shape[1] == (h * (1 + 3 * wout) + 15) // 16 * 16
    return body[:, :, 1:].reshape(r.shape[0], h, wout, 3)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_source_maps_equal_the_host_specification(ops, shape, name):
    d, k, kw, src, filled = _host(name, shape)
    got_src, got_filled = ops.stereo_source(torch.from_numpy(d).to(DEV), k, **kw)
    assert got_src.dtype == got_filled.dtype == torch.int32 and tuple(got_src.shape) == tuple(got_filled.shape) == shape
    assert np.array_equal(got_src.cpu().numpy(), src), int((got_src.cpu().numpy() != src).sum())
    assert np.array_equal(got_filled.cpu().numpy(), filled), int((got_filled.cpu().numpy() != filled).sum())
    if name == "tie" and shape[2] >= 3:
        assert src[0, -1, :3].tolist() == [0, 0, 0]  # the first pixel wins the third pixel's target
        assert shape[1] == 1 or ((src[0, 0] == -1).all() and (filled[0, 0] == -1).all())
    if name in ("steps", "random", "negative") and shape[2] >= 64:
        assert (src == -1).any() and (src >= 0).any() and (filled >= 0).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_equal_the_host_bytes(ops, shape, layout):
    from patchrefinerv2_amd.output import stereo_image_host
    B, h, w = shape
    for name in ("random", "steps"):
        d, k, kw, _, _ = _host(name, shape)
        img = np.stack([_image(h, w, f) for f in range(B)])
        want = np.stack([stereo_image_host(d[f], img[f], k, layout=layout, **kw) for f in range(B)])
        rows = ops.stereo_rows(torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV), k, layout=layout, **kw)
        got = _rows_to_image(rows, h, want.shape[2])
        assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_an_image_of_another_size_is_sampled_nearest(ops):
    from patchrefinerv2_amd.output import stereo_image_host
    shape = (2, 7, 83)
    d, k, kw, _, _ = _host("steps", shape)
    for hi, wi in ((3, 200), (20, 31), (1, 1)):
        img = np.stack([_image(hi, wi, 7), _image(hi, wi, 8)])
        for layout in LAYOUTS:
            want = np.stack([stereo_image_host(d[f], img[f], k, layout=layout, **kw) for f in range(2)])
            rows = ops.stereo_rows(torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV), k, layout=layout, **kw)
            assert np.array_equal(_rows_to_image(rows, 7, want.shape[2]), want), (hi, wi, layout)
    one = ops.stereo_rows(torch.from_numpy(d[1]).to(DEV), torch.from_numpy(_image(20, 31, 8)).to(DEV), k, **kw)  # [h, w] and [3, hi, wi]
    two = ops.stereo_rows(torch.from_numpy(d).to(DEV), torch.from_numpy(np.stack([_image(20, 31, 7), _image(20, 31, 8)])).to(DEV), k, **kw)
    assert torch.equal(one[0], two[1])  # a frame of a batch equals the frame alone


def test_a_row_wider_than_4096_columns(ops):
    """the second instance of the kernel (rows of 4097 .. 8192 columns; 32 columns per lane)"""
    from patchrefinerv2_amd.output import stereo_image_host
    shape = (1, 2, 4100)
    d, k, kw, src, filled = _host("steps", shape)
    got = ops.stereo_source(torch.from_numpy(d).to(DEV), k, **kw)
    assert np.array_equal(got[0].cpu().numpy(), src) and np.array_equal(got[1].cpu().numpy(), filled) and (src == -1).any()
    img = _image(2, 50, 3)
    rows = ops.stereo_rows(torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV), k, layout="sbs", **kw)
    assert np.array_equal(_rows_to_image(rows, 2, 8200)[0], stereo_image_host(d[0], img, k, layout="sbs", **kw))


def test_determinism_and_validation(ops):
    shape = (1, 6, 257)
    d, k, kw, _, _ = _host("random", shape)
    dd, img = torch.from_numpy(d).to(DEV), torch.from_numpy(_image(6, 257, 1)).to(DEV)
    a, b = ops.stereo_rows(dd, img, k, layout="sbs", **kw), ops.stereo_rows(dd, img, k, layout="sbs", **kw)
    assert torch.equal(a, b)
    assert all(torch.equal(x, y) for x, y in zip(ops.stereo_source(dd, k, **kw), ops.stereo_source(dd, k, **kw)))
    limit = ops.L.load().prv2_stereo_max_width()
    assert limit >= 8192
    wide = torch.ones((1, 1, limit + 1), device=DEV)
    with pytest.raises(ValueError, match=str(limit)):
        ops.stereo_source(wide, k, 0.1)
    with pytest.raises(ValueError, match=str(limit)):
        ops.stereo_rows(wide, torch.ones((3, 1, 4), device=DEV), k, 0.1)
    with pytest.raises(ValueError):
        ops.stereo_source(dd.cpu(), k, 0.1)
    with pytest.raises(ValueError):
        ops.stereo_rows(dd.cpu(), img, k, 0.1)
    with pytest.raises(ValueError):
        ops.stereo_rows(dd, img.cpu(), k, 0.1)
    for bad in (dict(baseline=INF), dict(baseline=0.1, convergence=0.0), dict(baseline=0.1, convergence=float("nan")),
                dict(baseline=0.1, edge_thr=float("nan")), dict(baseline=0.1, depth_range=(float("nan"), 1.0)), dict(baseline=0.1, layout="left")):
        with pytest.raises(ValueError):
            ops.stereo_rows(dd, img, k, **bad)
    with pytest.raises(ValueError):
        ops.stereo_rows(dd, torch.ones(2, 3, 4, 5, device=DEV), k, 0.1)


# ------------------------------------------------------------------------------------------------------------------ OutputStage
def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


@pytest.mark.parametrize("device_deflate", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_output_stage_writes_the_host_routes_view(tmp_path, layout, device_deflate):
    from patchrefinerv2_amd.output import OutputStage, write_geometry_host
    shape = (1, 7, 83)
    d, k, kw, _, _ = _host("steps", shape)
    img = _image(30, 41, 11)
    geo = dict(depth_range=kw["depth_range"], edge_thr=kw["edge_thr"])
    stereo = dict(baseline=kw["baseline"], convergence=kw["convergence"], layout=layout)
    (tmp_path / "host").mkdir()
    write_geometry_host(str(tmp_path / "host" / "f"), d[0], img, k, ply=False, normals=True, stereo=stereo, **geo)
    host = _files(tmp_path / "host")
    assert set(host) == {"f_normal.png", f"f_{layout}.png"}

    def run(work, **more):
        stage = OutputStage(str(tmp_path / work), workers=2, device_deflate=device_deflate)
        stage.submit_geometry(os.path.join(str(tmp_path / work), "f"), torch.from_numpy(d[0]).to(DEV), torch.from_numpy(img), k, ply=False,
                              normals=True, **geo, **more)
        stage.close()
        return _files(tmp_path / work), stage

    dev, stage = run("dev", stereo=stereo)
    assert set(dev) == set(host)
    for n in host:
        assert np.array_equal(_decode(dev[n]), _decode(host[n])), n
        assert device_deflate or dev[n] == host[n], n  # the same container and deflate: the same file
    off, stage_off = run("off")
    assert set(off) == {"f_normal.png"} and np.array_equal(_decode(off["f_normal.png"]), _decode(host["f_normal.png"]))
    assert stage.files - stage_off.files == 1
    if not device_deflate:
        wout = 83 * (2 if layout == "sbs" else 1)
        assert stage.bytes_d2h - stage_off.bytes_d2h == (7 * (1 + 3 * wout) + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------------------------ Tester
@pytest.mark.parametrize("mode", ["m1", "r4"])
def test_tester_run_writes_the_host_routes_view(tmp_path, mode):
    """Tester.run --save --device-output --save-stereo against the host route, for an m-mode (the result has the re-ensemble shape:
    the intrinsics are scaled) and an r-mode; and without the flag the files from before"""
    from patchrefinerv2_amd import models, weights as W  # noqa: F401  (registers the model classes)
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.tester import ImageDataset, RunnerInfo, Tester
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    name = "v1_dav2s_1080p_m1"  # (the smallest run of tests/test_output_gpu.py)
    w = WORKLOADS[name]
    (tmp_path / "imgs").mkdir()
    np.save(str(tmp_path / "imgs" / "f0.npy"), np.random.RandomState(60).rand(90, 160, 3).astype(np.float32))
    m = build_model(model_config(name, prec="bf16x3", max_batch=int(w.get("max_batch", 41)), n_streams=3))
    m.load_state_dict(W.synth_state_dict(state_spec(name), seed=0), strict=True)
    ds = ImageDataset(str(tmp_path / "imgs"), min_depth=1e-3, max_depth=80, image_resolution=w["raw"])
    geo = dict(save_stereo=True, fov=70.0, ply_edge_thr=0.05, ply_depth_range=(0.0, float("inf")), stereo_baseline=0.5, stereo_convergence=40.0,
               stereo_layout="anaglyph")

    def run(work, **info):
        t = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path / work), output_workers=4, **info), ds, m)
        res = t.run(cai_mode=mode, image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621)
        return _files(tmp_path / work), t.last_output_stage, res

    host, _, res = run("host", **geo)
    dev, stage, _ = run("dev", device_output=True, **geo)
    off, stage_off, _ = run("off", device_output=True)
    rh, rw = res[0]["shape"][-2:]
    assert (mode == "m1") == ((rh, rw) != tuple(w["raw"]))  # the m-mode's result is not at the raw shape
    assert set(dev) == set(host) == set(off) | {"f0_anaglyph.png"}
    assert dev["f0_anaglyph.png"] == host["f0_anaglyph.png"] and _decode(dev["f0_anaglyph.png"]).shape == (rh, rw, 3)
    assert {n: v for n, v in dev.items() if n != "f0_anaglyph.png"} == off
    assert stage.files - stage_off.files == 1 and stage.bytes_d2h - stage_off.bytes_d2h == (rh * (1 + 3 * rw) + 15) // 16 * 16


def test_cli_save_stereo_side_by_side(tmp_path):
    (tmp_path / "imgs").mkdir()
    np.save(str(tmp_path / "imgs" / "frame0.npy"), np.random.RandomState(20).rand(90, 160, 3).astype(np.float32))
    cfg = tmp_path / "cfg.py"
    cfg.write_text(f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n"
                   "model = dict(config=dict(patch_process_shape=[112, 224], image_raw_shape=[256, 512], patch_split_num=[2, 2],\n"
                   "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), str(cfg), "--synthetic-weights", "--cai-mode", "r4",
                        "--cfg-option", f"general_dataloader.dataset.rgb_image_dir={tmp_path / 'imgs'}", "--save", "--work-dir", str(out),
                        "--image-raw-shape", "256", "512", "--patch-split-num", "2", "2", "--device-output", "--save-stereo",
                        "--stereo-layout", "sbs"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "frame0_sbs.png" in os.listdir(out) and "frame0_right.png" not in os.listdir(out)
    sbs = _decode((out / "frame0_sbs.png").read_bytes())
    assert sbs.shape == (256, 2 * 512, 3) and sbs[:, :512].any()
