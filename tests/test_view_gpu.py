"""GPU: the novel-view export (csrc/view.hip through ops.view_source / ops.view_rows, OutputStage.submit_geometry(views=...)).  The
oracle is the host specification of patchrefinerv2_amd/output.py (numpy float32): the int32 source maps, the bits of the fp32 iz map
and the scanline bytes are compared for equality, on both dispatch routes.  The raster kernel owns a source tile of 64 x 16 pixels
per workgroup (the shapes sit on both sides of it in each direction); the resolve kernel a row of the view, in two instances (at most
4096 columns, and wider)."""
import io
import math
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
SHAPES = [(1, 1, 1), (1, 1, 2), (1, 2, 2), (1, 3, 7), (1, 5, 64), (1, 4, 65), (1, 17, 66), (1, 33, 130), (2, 7, 83)]  # frames, rows, columns
SCENES = ("steps", "slant", "random", "zoom", "behind")
POSES = ("identity", "circle", "dolly")
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


# scene name -> (depth [B, h, w], depth_range and edge_thr of the call, the amplitude of its circle, the translation of its dolly pose, a
# rotation about y)
def _scene(name, B, h, w):
    rs = np.random.RandomState(B * 1000 + h * 31 + w)
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    kw = dict(depth_range=(0.0, INF), edge_thr=0.05)
    circle, dolly, yaw = 0.15, (0.0, 0.0, -0.4), 0.0
    if name == "steps":  # blocks in front of a far wall: occlusions and hole runs beside them
        d = np.full((h, w), 6.0, dtype=F32)
        d[:, w // 6:w // 3] = 2.0
        d[h // 2:, w // 2:(3 * w) // 4] = 1.0
    elif name == "slant":  # a plane that stretches in the new view: faces of several pixels
        d = (1.0 + 4.0 * (w - x) / w + 0.05 * y).astype(F32)
        kw.update(edge_thr=0.5)
        circle = 0.4
    elif name == "random":  # random depth, 10 % invalid pixels of every kind, a finite depth range
        d = (1.0 + 5.0 * rs.rand(h, w)).astype(F32)
        idx = rs.choice(h * w, size=(h * w + 9) // 10, replace=False)
        d.reshape(-1)[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.0, -1.5, 0.2, 9.0], dtype=F32), idx.size)
        kw.update(depth_range=(0.5, 7.0), edge_thr=0.3)
    elif name == "zoom":  # two slanted planes that meet in a ridge at the middle column, 1 m away in the middle row; the dolly heads for
        d = (1.0 + 0.2 * np.abs(x - w // 2) / w + 0.02 * np.abs(y - h // 2)).astype(F32)  # that point and stops 5 cm in front of it:
        kw.update(edge_thr=0.0)                                                            # magnified 20-fold there, past the cap of 16
        fx, fy, cx, cy = (float(v) for v in _camera(h, w))
        dolly = (-(w // 2 + 0.5 - cx) / fx, -(h // 2 + 0.5 - cy) / fy, -0.95)
    elif name == "behind":  # the camera turns by 69 degrees: part of the scene is behind it or far off the frame
        d = (2.0 + 3.0 * rs.rand(h, w) * (x > w // 2) + 0.01 * x).astype(F32)
        kw.update(edge_thr=0.0)
        yaw = 1.2
    else:
        raise KeyError(name)
    d = np.stack([d] + [np.roll(d, 3 * f, axis=1) + F32(0.25 * f) for f in range(1, B)])
    return np.ascontiguousarray(d, dtype=F32), kw, circle, dolly, yaw


def _poses(kind, circle, dolly, yaw):
    """the poses of one call -> float32 [nv, 12]: the identity alone; three poses of a circle with a finite focus; one dolly pose (the
    eye forward by the scene's translation); a scene's rotation about y is applied after them (not to the identity)"""
    from patchrefinerv2_amd.output import IDENTITY_POSE, view_poses
    if kind == "identity":
        return np.array([IDENTITY_POSE], dtype=F32)
    p = view_poses(3, "circle", circle, 3.0) if kind == "circle" else np.array([[1, 0, 0, dolly[0], 0, 1, 0, dolly[1], 0, 0, 1, dolly[2]]], dtype=F32)
    if yaw:
        c, s = math.cos(yaw), math.sin(yaw)
        turn = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        p = np.stack([(turn @ m.astype(np.float64).reshape(3, 4)).reshape(12) for m in p]).astype(F32)
    return np.ascontiguousarray(p)


_HOST = {}


def _host(name, shape, kind):
    """the specification's maps of a scene, [B, nv, h, w] each, computed once and shared (never modified)"""
    from patchrefinerv2_amd.output import view_source_host
    key = (name, shape, kind)
    if key not in _HOST:
        d, kw, circle, dolly, yaw = _scene(name, *shape)
        k, poses = _camera(*shape[1:]), _poses(kind, circle, dolly, yaw)
        maps = [[view_source_host(d[f], k, p, **kw) for p in poses] for f in range(shape[0])]
        _HOST[key] = (d, k, poses, kw) + tuple(np.stack([np.stack([m[i] for m in per]) for per in maps]) for i in range(3))
    return _HOST[key]


def _rows_to_image(rows, h, w):
    """scanline buffers [B, nv, bytes] (a device tensor) -> uint8 [B, nv, h, w, 3]; every filter byte and the tail are zero"""
    r = rows.cpu().numpy()
    assert r.shape[2] == (h * (1 + 3 * w) + 15) // 16 * 16
    body = r[:, :, :h * (1 + 3 * w)].reshape(r.shape[0], r.shape[1], h, 1 + 3 * w)
    assert not body[..., 0].any() and not r[:, :, h * (1 + 3 * w):].any()
    return body[..., 1:].reshape(r.shape[0], r.shape[1], h, w, 3)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maps_equal_the_host_specification(ops, shape, name):
    from patchrefinerv2_amd.output import _view_vertices, view_source_host
    for kind in POSES:
        d, k, poses, kw, src, filled, iz = _host(name, shape, kind)
        got = ops.view_source(torch.from_numpy(d).to(DEV), k, poses, **kw)
        want_shape = (shape[0], len(poses), shape[1], shape[2])
        assert got[0].dtype == got[1].dtype == torch.int32 and got[2].dtype == torch.float32
        assert all(tuple(g.shape) == want_shape for g in got)
        for g, want, what in zip(got, (src, filled, iz), ("src", "filled", "iz")):
            g = g.cpu().numpy()
            assert np.array_equal(g.view(np.int32), want.view(np.int32)), (kind, what, int((g.view(np.int32) != want.view(np.int32)).sum()))
        # the scenes do their work
        if kind == "identity":
            valid = np.isfinite(d) & (d > F32(kw["depth_range"][0])) & (d < F32(kw["depth_range"][1]))
            assert np.array_equal(src[:, 0] >= 0, valid)
        elif shape[2] >= 64:
            if name in ("steps", "random"):
                assert (src == -1).any() and (src >= 0).any()
                assert (filled >= 0).all()
            if name == "zoom" and kind == "dolly":  # holes that exist only because of the cap
                loose = np.stack([view_source_host(d[f], k, poses[0], max_face=64, **kw)[0] for f in range(shape[0])])
                assert ((src[:, 0] == -1) & (loose >= 0)).any() and ((src[:, 0] >= 0) <= (loose >= 0)).all()
            if name == "behind":
                seen = np.stack([_view_vertices(d[f], k, poses[0], kw["depth_range"])[1] for f in range(shape[0])])
                assert not seen.all() and seen.any()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rows_equal_the_host_bytes(ops, shape):
    from patchrefinerv2_amd.output import view_image_host
    B, h, w = shape
    for name, kind in (("random", "circle"), ("steps", "dolly"), ("zoom", "dolly")):
        d, k, poses, kw, _, _, _ = _host(name, shape, kind)
        img = np.stack([_image(h, w, f) for f in range(B)])
        want = np.stack([np.stack([view_image_host(d[f], img[f], k, p, **kw) for p in poses]) for f in range(B)])
        rows = ops.view_rows(torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV), k, poses, **kw)
        got = _rows_to_image(rows, h, w)
        assert np.array_equal(got, want), (name, int((got != want).sum()))


def test_an_image_of_another_size_is_sampled_nearest(ops):
    from patchrefinerv2_amd.output import view_image_host
    shape = (2, 7, 83)
    d, k, poses, kw, _, _, _ = _host("steps", shape, "circle")
    for hi, wi in ((3, 200), (20, 31), (1, 1)):
        img = np.stack([_image(hi, wi, 7), _image(hi, wi, 8)])
        want = np.stack([np.stack([view_image_host(d[f], img[f], k, p, **kw) for p in poses]) for f in range(2)])
        rows = ops.view_rows(torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV), k, poses, **kw)
        assert np.array_equal(_rows_to_image(rows, 7, 83), want), (hi, wi)
    one = ops.view_rows(torch.from_numpy(d[1]).to(DEV), torch.from_numpy(_image(20, 31, 8)).to(DEV), k, poses[1], **kw)  # [h, w], [3, hi, wi], [12]
    two = ops.view_rows(torch.from_numpy(d).to(DEV), torch.from_numpy(np.stack([_image(20, 31, 7), _image(20, 31, 8)])).to(DEV), k, poses, **kw)
    assert tuple(one.shape) == (1, 1, two.shape[2]) and torch.equal(one[0, 0], two[1, 1])  # a frame and a view of a batch equal them alone


def test_a_row_wider_than_4096_columns(ops):
    """the second instance of the resolve kernel (rows of 4097 .. 8192 columns; 32 columns per lane)"""
    from patchrefinerv2_amd.output import view_image_host
    shape = (1, 2, 4100)
    d, k, poses, kw, src, filled, iz = _host("steps", shape, "circle")
    got = ops.view_source(torch.from_numpy(d).to(DEV), k, poses, **kw)
    for g, want in zip(got, (src, filled, iz)):
        assert np.array_equal(g.cpu().numpy().view(np.int32), want.view(np.int32))
    assert (src == -1).any()
    img = _image(2, 50, 3)
    rows = ops.view_rows(torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV), k, poses, **kw)
    assert np.array_equal(_rows_to_image(rows, 2, 4100)[0], np.stack([view_image_host(d[0], img, k, p, **kw) for p in poses]))


def test_determinism_and_validation(ops):
    shape = (1, 17, 66)
    d, k, poses, kw, _, _, _ = _host("random", shape, "circle")
    dd, img = torch.from_numpy(d).to(DEV), torch.from_numpy(_image(17, 66, 1)).to(DEV)
    assert torch.equal(ops.view_rows(dd, img, k, poses, **kw), ops.view_rows(dd, img, k, poses, **kw))
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32))
               for x, y in zip(ops.view_source(dd, k, poses, **kw), ops.view_source(dd, k, poses, **kw)))
    assert all(torch.equal(x, y) for x, y in zip(ops.view_source(dd, k, torch.from_numpy(poses).to(DEV), **kw), ops.view_source(dd, k, poses, **kw)))
    for bad in (np.zeros((3, 4), F32), np.zeros((2, 3, 4), F32), np.zeros((0, 12), F32), np.zeros((11,), F32)):  # a pose array of the wrong shape
        with pytest.raises(ValueError, match="poses"):
            ops.view_source(dd, k, bad, **kw)
        with pytest.raises(ValueError, match="poses"):
            ops.view_rows(dd, img, k, bad, **kw)
    with pytest.raises(ValueError, match="device"):  # a depth map on another device than the image
        ops.view_rows(dd, img.cpu(), k, poses, **kw)
    with pytest.raises(ValueError):
        ops.view_rows(dd.cpu(), img, k, poses, **kw)
    with pytest.raises(ValueError):
        ops.view_source(dd.cpu(), k, poses, **kw)
    limit = ops.L.load().prv2_stereo_max_width()
    wide = torch.ones((1, 1, limit + 1), device=DEV)
    with pytest.raises(ValueError, match=str(limit)):  # a row past prv2_stereo_max_width()
        ops.view_source(wide, k, poses)
    with pytest.raises(ValueError, match=str(limit)):
        ops.view_rows(wide, torch.ones((3, 1, 4), device=DEV), k, poses)
    big = torch.empty((1, 4096, 4096), device=DEV)  # 2^24 pixels: 32 views reach 2^29
    with pytest.raises(ValueError, match="2\\^29"):
        ops.view_source(big, k, np.zeros((32, 12), F32))
    with pytest.raises(ValueError, match="2\\^29"):
        ops.view_rows(big, torch.ones((3, 1, 4), device=DEV), k, np.zeros((32, 12), F32))
    del big
    for bad in (dict(edge_thr=float("nan")), dict(depth_range=(float("nan"), 1.0))):
        with pytest.raises(ValueError):
            ops.view_source(dd, k, poses, **bad)
    with pytest.raises(ValueError):
        ops.view_source(dd, (0.0, 5.0, 1.0, 1.0), poses)
    with pytest.raises(ValueError):
        ops.view_rows(dd, torch.ones(2, 3, 4, 5, device=DEV), k, poses)


# ------------------------------------------------------------------------------------------------------------------ OutputStage
def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


@pytest.mark.parametrize("device_deflate", [False, True])
def test_output_stage_writes_the_host_routes_views(tmp_path, device_deflate):
    """five views: a chunk of four and a chunk of one, each in a staging slot of its own"""
    from patchrefinerv2_amd.output import OutputStage, write_geometry_host
    shape = (1, 7, 83)
    d, k, _, kw, _, _, _ = _host("steps", shape, "circle")
    img = _image(30, 41, 11)
    views = dict(count=5, motion="circle", amplitude=0.2, focus=4.0)
    (tmp_path / "host").mkdir()
    write_geometry_host(str(tmp_path / "host" / "f"), d[0], img, k, ply=False, normals=True, views=views, **kw)
    host = _files(tmp_path / "host")
    assert set(host) == {"f_normal.png"} | {f"f_view_{i:03d}.png" for i in range(5)}

    def run(work, **more):
        stage = OutputStage(str(tmp_path / work), workers=2, device_deflate=device_deflate)
        stage.submit_geometry(os.path.join(str(tmp_path / work), "f"), torch.from_numpy(d[0]).to(DEV), torch.from_numpy(img), k, ply=False,
                              normals=True, **kw, **more)
        stage.close()
        return _files(tmp_path / work), stage

    dev, stage = run("dev", views=views)
    assert set(dev) == set(host)
    for n in host:
        assert np.array_equal(_decode(dev[n]), _decode(host[n])), n
        assert device_deflate or dev[n] == host[n], n  # the same container and deflate: the same file
    assert len({dev[f"f_view_{i:03d}.png"] for i in range(5)}) == 5
    off, stage_off = run("off")
    assert set(off) == {"f_normal.png"} and off["f_normal.png"] == dev["f_normal.png"]
    assert stage.files - stage_off.files == 5
    if not device_deflate:
        assert stage.bytes_d2h - stage_off.bytes_d2h == 5 * ((7 * (1 + 3 * 83) + 15) // 16 * 16)


# ------------------------------------------------------------------------------------------------------------------ Tester
def test_tester_run_writes_the_views(tmp_path, monkeypatch):
    """Tester.run --save --device-output with save_views=3, an m-mode (the result has the re-ensemble shape: the intrinsics are scaled):
    three more files, the pixels of ops.view_rows for the map, camera and path the tester handed to the output stage (the kernel is
    pinned to the specification above; tools/test.py's two routes are compared below); without the flag the files from before"""
    from patchrefinerv2_amd import models, ops, output as O, weights as W  # noqa: F401  (registers the model classes)
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
    geo = dict(save_views=3, view_motion="circle", view_amplitude=0.5, view_focus=40.0, fov=70.0, ply_edge_thr=0.05, ply_depth_range=(0.0, float("inf")))
    seen = []
    submit = O.OutputStage.submit_geometry

    def spy(self, base, result, image_hr, intrinsics, **kw):
        if kw.get("views") is not None:
            seen.append((result.clone(), torch.as_tensor(image_hr).clone(), np.array(intrinsics), dict(kw)))
        return submit(self, base, result, image_hr, intrinsics, **kw)
    monkeypatch.setattr(O.OutputStage, "submit_geometry", spy)

    def run(work, **info):
        t = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path / work), output_workers=4, device_output=True, **info), ds, m)
        res = t.run(cai_mode="m1", image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621)
        return _files(tmp_path / work), t.last_output_stage, res

    dev, stage, res = run("dev", **geo)
    off, stage_off, _ = run("off")
    rh, rw = res[0]["shape"][-2:]
    names = {f"f0_view_{i:03d}.png" for i in range(3)}
    assert (rh, rw) != tuple(w["raw"]) and set(dev) == set(off) | names and {n: v for n, v in dev.items() if n not in names} == off
    assert stage.files - stage_off.files == 3 and stage.bytes_d2h - stage_off.bytes_d2h == 3 * ((rh * (1 + 3 * rw) + 15) // 16 * 16)
    assert len(seen) == 1
    result, image, k, kw = seen[0]
    assert kw["views"] == dict(count=3, motion="circle", amplitude=0.5, focus=40.0)
    assert np.array_equal(k, O.camera_intrinsics(w["raw"], (rh, rw), fov=70.0))
    img = image[0] if image.dim() == 4 else image
    rows = ops.view_rows(result.reshape(rh, rw).to(DEV), img.to(DEV), k, O.view_poses(**kw["views"]), kw["depth_range"], kw["edge_thr"])
    want = _rows_to_image_one(rows, rh, rw)
    for i in range(3):
        assert np.array_equal(_decode(dev[f"f0_view_{i:03d}.png"]), want[i]), i
    assert not np.array_equal(want[0], want[1])


def _rows_to_image_one(rows, h, w):
    r = rows.cpu().numpy()[0]
    return r[:, :h * (1 + 3 * w)].reshape(r.shape[0], h, 1 + 3 * w)[:, :, 1:].reshape(r.shape[0], h, w, 3)


def test_cli_save_views(tmp_path):
    """tools/test.py --save --device-output --save-views in a fresh process writes the specification's pixels: the same run on the host
    route (the same model, weights and frame: the same map) writes the files from view_image_host itself (tests/test_view_host.py
    pins those files to the specification)"""
    (tmp_path / "imgs").mkdir()
    np.save(str(tmp_path / "imgs" / "frame0.npy"), np.random.RandomState(20).rand(90, 160, 3).astype(np.float32))
    cfg = tmp_path / "cfg.py"
    cfg.write_text(f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n"
                   "model = dict(config=dict(patch_process_shape=[112, 224], image_raw_shape=[256, 512], patch_split_num=[2, 2],\n"
                   "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")

    def run(work, *route):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), str(cfg), "--synthetic-weights", "--cai-mode", "r4",
                            "--cfg-option", f"general_dataloader.dataset.rgb_image_dir={tmp_path / 'imgs'}", "--save", "--work-dir", str(tmp_path / work),
                            "--image-raw-shape", "256", "512", "--patch-split-num", "2", "2", *route, "--save-views", "2", "--view-motion", "circle",
                            "--view-amplitude", "0.5", "--view-focus", "30"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert sorted(n for n in os.listdir(tmp_path / work) if "_view_" in n) == ["frame0_view_000.png", "frame0_view_001.png"]
        return [_decode((tmp_path / work / f"frame0_view_{i:03d}.png").read_bytes()) for i in range(2)]

    dev, host = run("dev", "--device-output"), run("host")
    assert dev[0].shape == (256, 512, 3) and all(np.array_equal(a, b) for a, b in zip(dev, host))
    assert dev[0].any() and not np.array_equal(dev[0], dev[1])
