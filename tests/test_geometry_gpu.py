"""GPU: the geometry export (csrc/pointcloud.hip through ops.pointcloud_pack / ops.normal_rows, OutputStage.submit_geometry).  The
oracle is the host specification of patchrefinerv2_amd/output.py (numpy float32): vertex bytes, counts and scanline bytes are compared
for equality, on both dispatch routes.  A block of the count / pack kernels owns a run of RUN = 2048 pixels (kRun in
csrc/pointcloud.hip): the shapes below are one pixel, a width that is no multiple of 4, and 61 x 83 = 5063 pixels = two full runs and a
ragged third."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
RUN = 2048
F32 = np.float32
SENTINEL = 0xA5
torch.set_grad_enabled(False)


@pytest.fixture(params=["torch", "ctypes"])
def ops(request, monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    monkeypatch.setattr(ops, "DISPATCH", request.param)
    return ops


def _camera(h, w):
    from patchrefinerv2_amd.output import camera_intrinsics
    return camera_intrinsics((h, w), (h, w), fov=63.0) + F32(0.37)  # (off-centre principal point, fx != fy)


def _depth(h, w, seed, holes=True):
    """a smooth surface with a step (flying pixels at the default threshold), noise, and every kind of invalid value"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    d = (2.0 + 3.0 * (x > 0.55 * w) + 0.03 * x + 0.02 * y + 0.05 * rs.rand(h, w)).astype(F32)
    if holes and h * w > 8:
        flat = d.reshape(-1)
        idx = rs.choice(h * w, size=max(5, h * w // 23), replace=False)
        flat[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.0, -1.5], dtype=F32), idx.size)
    return d


def _image(hi, wi, seed):
    img = np.random.RandomState(100 + seed).rand(3, hi, wi).astype(F32) * F32(1.2) - F32(0.1)  # below 0 and above 1 clamp
    img.reshape(-1)[::31] = np.nan
    return img


def _check_cloud(ops, depth, image, k, **kw):
    """depth [B, h, w], image [B, 3, hi, wi] (numpy): every frame's bytes and count against pointcloud_host; the bytes behind the
    records must keep the sentinel the buffer was filled with -> the counts"""
    from patchrefinerv2_amd.output import pointcloud_host
    B, h, w = depth.shape
    stride = kw.get("stride", 1)
    bound = 15 * math.ceil(h / stride) * math.ceil(w / stride)
    out = torch.full((B, bound + 37), SENTINEL, dtype=torch.uint8, device=DEV)
    verts, counts = ops.pointcloud_pack(torch.from_numpy(depth).to(DEV), torch.from_numpy(image).to(DEV), k, out=out, **kw)
    assert verts is out and counts.dtype == torch.int64 and tuple(counts.shape) == (B,)
    got, counts = out.cpu().numpy(), counts.cpu().numpy()
    for f in range(B):
        want = pointcloud_host(depth[f], image[f], k, **kw)
        assert counts[f] == want.size, (f, counts[f], want.size)
        nb = 15 * want.size
        assert got[f, :nb].tobytes() == want.tobytes(), (f, int((got[f, :nb] != np.frombuffer(want.tobytes(), np.uint8)).sum()))
        assert (got[f, nb:] == SENTINEL).all(), f
    # without ``out``: a buffer of exactly the bound
    verts2, counts2 = ops.pointcloud_pack(torch.from_numpy(depth).to(DEV), torch.from_numpy(image).to(DEV), k, **kw)
    assert tuple(verts2.shape) == (B, bound) and np.array_equal(counts2.cpu().numpy(), counts)
    for f in range(B):
        assert np.array_equal(verts2[f, :15 * counts[f]].cpu().numpy(), got[f, :15 * counts[f]])
    return counts


def _check_normals(ops, depth, k, **kw):
    from patchrefinerv2_amd.output import normal_map_host
    B, h, w = depth.shape
    rows = ops.normal_rows(torch.from_numpy(depth).to(DEV), k, **kw).cpu().numpy()
    n = h * (1 + 3 * w)
    assert rows.shape == (B, (n + 15) // 16 * 16)
    for f in range(B):
        want = np.zeros((h, 1 + 3 * w), dtype=np.uint8)
        want[:, 1:] = normal_map_host(depth[f], k, **kw).reshape(h, 3 * w)
        assert np.array_equal(rows[f, :n].reshape(h, 1 + 3 * w), want), (f, int((rows[f, :n].reshape(h, -1) != want).sum()))
        assert not rows[f, n:].any()


@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (61, 83)])
def test_cloud_and_normals_equal_the_host_specification(ops, shape):
    h, w = shape
    assert (h, w) != (61, 83) or (h * w > 2 * RUN and h * w % RUN != 0)  # three blocks, the last one ragged
    d = _depth(h, w, seed=h, holes=True)[None]
    if (h, w) == (1, 1):
        d[:] = 2.0
    k = _camera(h, w)
    n = _check_cloud(ops, d, _image(h, w, 1)[None], k)
    assert (h, w) == (1, 1) and n[0] == 1 or 0 < n[0] < h * w
    _check_normals(ops, d, k)


def test_many_pixels_catch_a_last_bit_difference(ops):
    """480 x 640 on a smooth map: a square root or division that is off by one ulp moves a byte of the normal map only where a
    component lands next to a rounding boundary, about once in 1e5 pixels -- too rare for the small shapes above to see"""
    h, w = 480, 640
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    d = (4.0 + 0.8 * np.sin(x / 41.0) * np.cos(y / 29.0) + 0.002 * x + 0.001 * np.random.RandomState(9).rand(h, w)).astype(F32)[None]
    k = _camera(h, w)
    _check_normals(ops, d, k)
    _check_cloud(ops, d, _image(h, w, 9)[None], k, stride=2)


def test_two_frame_batch_with_different_counts(ops):
    h, w = 45, 67  # 3015 pixels: two runs per frame
    d = np.stack([_depth(h, w, 1), _depth(h, w, 2)])
    d[1, 10:30] = np.nan
    k = _camera(h, w)
    n = _check_cloud(ops, d, np.stack([_image(20, 31, 1), _image(20, 31, 2)]), k)
    assert n[0] != n[1] and n.min() > 0
    _check_normals(ops, d, k)
    # a frame of a batch equals the frame alone
    one, c1 = ops.pointcloud_pack(torch.from_numpy(d[1]).to(DEV), torch.from_numpy(_image(20, 31, 2)).to(DEV), k)
    two, c2 = ops.pointcloud_pack(torch.from_numpy(d).to(DEV), torch.from_numpy(np.stack([_image(20, 31, 1), _image(20, 31, 2)])).to(DEV), k)
    assert int(c1[0]) == int(c2[1]) and torch.equal(one[0, :15 * int(c1[0])], two[1, :15 * int(c1[0])])


@pytest.mark.parametrize("k_first", list(range(1, 17)) + [2047, 2048])
def test_seams_at_every_byte_alignment(ops, k_first):
    """the first block keeps k points, so the second block's byte range starts at 15 k: k = 1 .. 16 gives every residue mod 4 (and
    mod 16, the width of the interior stores); 2047 / 2048: a (nearly) full first run.  Every byte of the buffer is compared, the
    ones behind 15 N with the sentinel."""
    h, w = 61, 83
    rs = np.random.RandomState(k_first)
    d = (3.0 + 0.01 * rs.rand(h, w)).astype(F32)
    flat = d.reshape(-1)
    drop = np.ones(RUN, dtype=bool)
    drop[rs.choice(RUN, size=k_first, replace=False)] = False
    flat[:RUN][drop] = 0.0
    from patchrefinerv2_amd.output import keep_mask_host
    assert keep_mask_host(d).reshape(-1)[:RUN].sum() == k_first and keep_mask_host(d).reshape(-1)[RUN:].all()
    n = _check_cloud(ops, d[None], _image(h, w, 3)[None], _camera(h, w))
    assert n[0] == k_first + h * w - RUN


def test_masks_and_options(ops):
    h, w = 50, 47  # 2350 pixels: two runs
    k = _camera(h, w)
    img = _image(h, w, 4)[None]
    nothing = np.full((1, h, w), np.nan, dtype=F32)
    assert _check_cloud(ops, nothing, img, k)[0] == 0
    _check_normals(ops, nothing, k)
    d = _depth(h, w, 5, holes=False)[None]
    assert _check_cloud(ops, d, img, k, edge_thr=0.0)[0] == h * w  # all valid, filter off
    n_on = _check_cloud(ops, d, img, k, edge_thr=0.05)[0]
    assert 0 < n_on < h * w  # the step is dropped
    for stride in (1, 2, 3):
        n = _check_cloud(ops, d, img, k, edge_thr=0.0, stride=stride)[0]
        assert n == math.ceil(h / stride) * math.ceil(w / stride)
        _check_cloud(ops, _depth(h, w, 6)[None], img, k, stride=stride)  # filter on, with holes: full-resolution neighbours
    lo, hi = float(np.percentile(d, 20)), float(np.percentile(d, 80))
    n = _check_cloud(ops, d, img, k, depth_range=(lo, hi), edge_thr=0.0)[0]
    assert 0.5 * h * w < n < 0.7 * h * w  # both ends cut
    _check_normals(ops, d, k, depth_range=(lo, hi))
    _check_cloud(ops, d, _image(33, 71, 7)[None], k)  # an image of another size, ratios 0.66 and 1.51


def test_determinism(ops):
    h, w = 61, 83
    d, img, k = torch.from_numpy(_depth(h, w, 8)[None]).to(DEV), torch.from_numpy(_image(40, 50, 8)[None]).to(DEV), _camera(h, w)
    a, na = ops.pointcloud_pack(d, img, k, out=torch.zeros((1, 15 * h * w), dtype=torch.uint8, device=DEV))
    b, nb = ops.pointcloud_pack(d, img, k, out=torch.zeros((1, 15 * h * w), dtype=torch.uint8, device=DEV))
    assert torch.equal(a, b) and torch.equal(na, nb)
    assert torch.equal(ops.normal_rows(d, k), ops.normal_rows(d, k))


def test_wrappers_validate_their_arguments(ops):
    d, img, k = torch.ones(1, 4, 5, device=DEV), torch.ones(1, 3, 4, 5, device=DEV), [5.0, 5.0, 2.5, 2.0]
    for bad in (dict(stride=0), dict(edge_thr=float("nan")), dict(depth_range=(float("nan"), 1.0)),
                dict(out=torch.zeros((1, 15 * 20 - 1), dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            ops.pointcloud_pack(d, img, k, **bad)
    with pytest.raises(ValueError):
        ops.pointcloud_pack(d, torch.ones(2, 3, 4, 5, device=DEV), k)
    with pytest.raises(ValueError):
        ops.pointcloud_pack(d, img.cpu(), k)
    with pytest.raises(ValueError):
        ops.normal_rows(d, [0.0, 5.0, 2.5, 2.0])


def test_the_exports_share_one_wording_of_the_shared_checks(ops):
    """pointcloud_pack, stereo_rows, bokeh_rows and view_rows make one check of the image and of edge_thr (ops._scene_inputs), not four:
    the same wrong argument gets the same message behind the op's name"""
    d, img, k = torch.ones(1, 4, 5, device=DEV), torch.ones(1, 3, 4, 5, device=DEV), [5.0, 5.0, 2.5, 2.0]
    pose = np.eye(4, dtype=F32)[:3].reshape(12)
    calls = {"pointcloud_pack": lambda image, **kw: ops.pointcloud_pack(d, image, k, **kw),
             "stereo_rows": lambda image, **kw: ops.stereo_rows(d, image, k, 0.1, **kw),
             "view_rows": lambda image, **kw: ops.view_rows(d, image, k, pose, **kw),
             "bokeh_rows": lambda image, **kw: ops.bokeh_rows(d, image, k, **kw)}

    def messages(names, image, **kw):
        out = []
        for name in names:
            with pytest.raises(ValueError) as e:
                calls[name](image, **kw)
            assert str(e.value).startswith(name + ": ")
            out.append(str(e.value)[len(name) + 2:])
        return out

    for image in (torch.ones(2, 3, 4, 5, device=DEV), img.cpu()):
        got = messages(list(calls), image)
        assert len(set(got)) == 1 and "image" in got[0], got
    got = messages(list(calls)[:3], img, edge_thr=float("nan"))  # (the depth of field takes no threshold)
    assert len(set(got)) == 1 and "edge_thr" in got[0], got


# ------------------------------------------------------------------------------------------------------------------ Tester
def _model_and_data(tmp_path):
    from patchrefinerv2_amd import models, weights as W  # noqa: F401  (registers the model classes)
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.tester import ImageDataset
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    name = "v1_dav2s_1080p_m1"  # (the smallest run of tests/test_output_gpu.py)
    w = WORKLOADS[name]
    (tmp_path / "imgs").mkdir()
    for i in range(2):
        np.save(str(tmp_path / "imgs" / f"f{i}.npy"), np.random.RandomState(60 + i).rand(90, 160, 3).astype(np.float32))
    m = build_model(model_config(name, prec="bf16x3", max_batch=int(w.get("max_batch", 41)), n_streams=3))
    m.load_state_dict(W.synth_state_dict(state_spec(name), seed=0), strict=True)
    return m, ImageDataset(str(tmp_path / "imgs"), min_depth=1e-3, max_depth=80, image_resolution=w["raw"]), w


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _decode(data):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def _idat_bytes(png):
    import struct
    assert png[12:16] == b"IHDR" and png[37:41] == b"IDAT"
    return struct.unpack(">I", png[33:37])[0]


def _ply_count(data):
    from patchrefinerv2_amd.output import PLY_VERTEX, ply_header
    n = int(data.split(b"element vertex ", 1)[1].split(b"\n", 1)[0])
    assert data.startswith(ply_header(n)) and len(data) == len(ply_header(n)) + PLY_VERTEX.itemsize * n
    return n


@pytest.mark.parametrize("mode", ["m1", "r4"])
def test_tester_run_writes_the_host_routes_geometry(tmp_path, mode):
    """Tester.run --save --device-output --save-ply --save-normals against the host route, for an m-mode (the result has the
    re-ensemble shape: the intrinsics are scaled) and an r-mode; again with --device-deflate; and without the new flags"""
    from patchrefinerv2_amd import lib as L
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    m, ds, w = _model_and_data(tmp_path)
    geo = dict(save_ply=True, save_normals=True, fov=70.0, ply_stride=3, ply_edge_thr=0.05, ply_depth_range=(0.0, float("inf")))
    call = dict(cai_mode=mode, image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621)

    def run(work, fb=1, **info):
        t = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path / work), output_workers=4, **info), ds, m)
        res = t.run(**call, frame_batch=fb)
        return _files(tmp_path / work), t.last_output_stage, res

    host, _, res = run("host", **geo)
    names = {f"f{i}{s}" for i in range(2) for s in (".png", "_uint16.png", "_edge.png", "_coarse.png", ".ply", "_normal.png")}
    assert set(host) == names
    counts = [_ply_count(host[f"f{i}.ply"]) for i in range(2)]
    rh, rw = res[0]["shape"][-2:]
    assert all(0 < n <= math.ceil(rh / 3) * math.ceil(rw / 3) for n in counts)
    assert (mode == "m1") == ((rh, rw) != tuple(w["raw"]))  # the m-mode's result is not at the raw shape
    assert _decode(host["f0_normal.png"]).shape == (rh, rw, 3) and _decode(host["f0_normal.png"]).any()

    dev, stage, _ = run("dev", device_output=True, **geo)
    assert set(dev) == names
    for i in range(2):
        assert dev[f"f{i}.ply"] == host[f"f{i}.ply"] and dev[f"f{i}_normal.png"] == host[f"f{i}_normal.png"], i
    rb = L.load().prv2_rows_bytes
    pngs = rb(rh, rw, 2) + 2 * rb(rh, rw, 3) + rb(rh, rw, 1) + rb(*w["raw"], 3)  # uint16, colour + normal, edge, coarse
    assert stage.files == 12 and stage.bytes_d2h == 2 * pngs + sum(15 * n + 8 for n in counts)

    defl, stage, _ = run("defl", device_output=True, device_deflate=True, **geo)
    assert set(defl) == names
    for i in range(2):
        assert defl[f"f{i}.ply"] == host[f"f{i}.ply"], i
        assert np.array_equal(_decode(defl[f"f{i}_normal.png"]), _decode(host[f"f{i}_normal.png"])), i
    streams = sum(_idat_bytes(v) + 8 for n, v in defl.items() if n.endswith(".png"))
    assert stage.files == 12 and stage.bytes_d2h == streams + sum(15 * n + 8 for n in counts)  # 15 N + 8 per cloud, not the bound

    # no side effects: a RunnerInfo as it was before the flags existed, and one with the flags at their defaults, write the
    # files of the flagged run minus the new ones, byte for byte (two frames per call: the geometry is made per frame)
    old = {n: v for n, v in dev.items() if not n.endswith((".ply", "_normal.png"))}
    plain, stage, _ = run("plain", device_output=True)
    assert plain == old and stage.files == 8
    off, _, _ = run("off", device_output=True, save_ply=False, save_normals=False, intrinsics=None, fov=None, ply_stride=1,
                    ply_edge_thr=0.05, ply_depth_range=(0.0, float("inf")))
    assert off == old
    fb2, _, _ = run("fb2", fb=2, device_output=True, **geo)
    assert fb2 == dev
