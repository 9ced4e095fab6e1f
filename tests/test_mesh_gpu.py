"""GPU: the mesh export (csrc/pointcloud.hip through ops.mesh_pack, OutputStage.submit_geometry(mesh=True)).  The oracle is the host
specification of patchrefinerv2_amd/output.py (numpy float32): vertex bytes, face bytes and both counts are compared for equality, on
both dispatch routes.  A block of the count / pack kernels owns a run of RUN = 2048 cells (kRun in csrc/pointcloud.hip): 61 x 83 has
60 x 82 = 4920 cells = two full runs and a ragged third."""
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


# (the recipes of tests/test_geometry_gpu.py)
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


def _step_depth(h, w, holes):
    """a step between two columns that a stride-3 grid straddles (x = 45 | 48): nodes on both sides survive the flying filter"""
    rs = np.random.RandomState(5)
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    d = (2.0 + 3.0 * (x >= 47) + 0.03 * x + 0.02 * y + 0.05 * rs.rand(h, w)).astype(F32)
    if holes:
        idx = rs.choice(h * w, size=h * w // 23, replace=False)
        d.reshape(-1)[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.0, -1.5], dtype=F32), idx.size)
    return d


def _cell_census(depth, **kw):
    """from the specification: per cell the number of kept corners, the faces it emits and, for four kept corners, its diagonal"""
    from patchrefinerv2_amd.output import keep_mask_host, mesh_faces_host
    s = kw.get("stride", 1)
    keep = keep_mask_host(depth, **kw)[::s, ::s]
    z = np.asarray(depth, dtype=F32)[::s, ::s]
    corners = keep[:-1, :-1].astype(int) + keep[:-1, 1:] + keep[1:, :-1] + keep[1:, 1:]
    with np.errstate(all="ignore"):
        ad = np.abs(z[:-1, :-1] - z[1:, 1:]) <= np.abs(z[:-1, 1:] - z[1:, :-1])
    # every candidate has a corner in its cell's top row and one in its left column: the cell is (min gy, min gx) of the three nodes
    faces = mesh_faces_host(depth, **kw)
    rank_to_node = np.flatnonzero(keep.reshape(-1))
    gw = keep.shape[1]
    gy, gx = np.divmod(rank_to_node[faces], gw)  # [M, 3] node coordinates
    cell = gy.min(axis=1) * (gw - 1) + gx.min(axis=1)
    per_cell = np.bincount(cell, minlength=corners.size).reshape(corners.shape)
    return corners, per_cell, ad, keep


def _check_mesh(ops, depth, image, k, **kw):
    """depth [B, h, w], image [B, 3, hi, wi] (numpy): every frame's vertex and face bytes and counts against the specification; the
    bytes behind the records keep the sentinel the buffers were filled with -> (N, M)"""
    from patchrefinerv2_amd.output import mesh_face_records, mesh_faces_host, pointcloud_host
    B, h, w = depth.shape
    stride = kw.get("stride", 1)
    gh, gw = math.ceil(h / stride), math.ceil(w / stride)
    vbound, fbound = 15 * gh * gw, 26 * (gh - 1) * (gw - 1)
    d, img = torch.from_numpy(depth).to(DEV), torch.from_numpy(image).to(DEV)
    out_v = torch.full((B, vbound + 37), SENTINEL, dtype=torch.uint8, device=DEV)
    out_f = torch.full((B, fbound + 37), SENTINEL, dtype=torch.uint8, device=DEV)
    verts, n, faces, m = ops.mesh_pack(d, img, k, out_vertices=out_v, out_faces=out_f, **kw)
    assert verts is out_v and faces is out_f
    assert n.dtype == m.dtype == torch.int64 and tuple(n.shape) == tuple(m.shape) == (B,)
    got_v, got_f, n, m = out_v.cpu().numpy(), out_f.cpu().numpy(), n.cpu().numpy(), m.cpu().numpy()
    for f in range(B):
        want_v = pointcloud_host(depth[f], image[f], k, **kw)
        want_f = mesh_face_records(mesh_faces_host(depth[f], **kw))
        assert n[f] == want_v.size and m[f] == want_f.size, (f, n[f], want_v.size, m[f], want_f.size)
        nv, nf = 15 * want_v.size, 13 * want_f.size
        assert got_v[f, :nv].tobytes() == want_v.tobytes(), f
        assert got_f[f, :nf].tobytes() == want_f.tobytes(), (f, int((got_f[f, :nf] != np.frombuffer(want_f.tobytes(), np.uint8)).sum()))
        assert (got_v[f, nv:] == SENTINEL).all() and (got_f[f, nf:] == SENTINEL).all(), f
    # without the out buffers: exactly the bounds, the same records; and the vertices are pointcloud_pack's
    verts2, n2, faces2, m2 = ops.mesh_pack(d, img, k, **kw)
    assert tuple(verts2.shape) == (B, vbound) and tuple(faces2.shape) == (B, fbound)
    assert np.array_equal(n2.cpu().numpy(), n) and np.array_equal(m2.cpu().numpy(), m)
    cloud, nc = ops.pointcloud_pack(d, img, k, **kw)
    assert np.array_equal(nc.cpu().numpy(), n)
    for f in range(B):
        assert np.array_equal(faces2[f, :13 * m[f]].cpu().numpy(), got_f[f, :13 * m[f]])
        assert np.array_equal(verts2[f, :15 * n[f]].cpu().numpy(), got_v[f, :15 * n[f]])
        assert torch.equal(cloud[f, :15 * n[f]], verts2[f, :15 * n[f]])
    return n, m


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (2, 2), (37, 53), (61, 83)])
def test_mesh_equals_the_host_specification(ops, shape):
    h, w = shape
    d = _depth(h, w, seed=h, holes=True)[None]
    if h * w <= 8:
        d[:] = 2.0
    if (h, w) == (61, 83):
        # two full runs of cells and a ragged third, by the kernel's own run constant: the workspace is the index map + one int32 per run
        lib = ops.L.load()
        runs = lib.prv2_mesh_workspace_bytes(1, h, w, 1) // 4 - h * w
        cells = (h - 1) * (w - 1)
        assert runs == 3 == math.ceil(cells / RUN) and cells > 2 * RUN and cells % RUN != 0
        # every (corner count, diagonal) case occurs
        corners, per_cell, ad, keep = _cell_census(d[0])
        assert ((corners == 4) & ad).sum() > 0 and ((corners == 4) & ~ad).sum() > 0
        three_ad = (corners == 3) & keep[:-1, :-1] & keep[1:, 1:]
        assert three_ad.sum() > 0 and ((corners == 3) & ~three_ad).sum() > 0
        assert per_cell[corners < 3].sum() == 0
    n, m = _check_mesh(ops, d, _image(h, w, 1)[None], _camera(h, w))
    if h * w == 1 or h == 1:
        assert m[0] == 0 and n[0] == h * w
    elif (h, w) == (2, 2):
        assert m[0] == 2 and n[0] == 4
    else:
        assert 0 < m[0] < 2 * (h - 1) * (w - 1)


@pytest.mark.parametrize("holes", [False, True])
def test_discontinuity_inside_a_cell_of_four_kept_corners(ops, holes):
    """stride 3 over a step: cells whose four corners are kept but whose edges across the step are not joined emit no face, or
    one face of two (at stride 1 the flying filter removes such corners, so the small shapes above never see this)"""
    h, w = 61, 83
    d = _step_depth(h, w, holes)
    corners, per_cell, _, _ = _cell_census(d, stride=3)
    assert ((corners == 4) & (per_cell == 0)).sum() > 0 and ((corners == 4) & (per_cell == 1)).sum() > 0
    _check_mesh(ops, d[None], _image(h, w, 2)[None], _camera(h, w), stride=3)


def test_no_filter_and_strides(ops):
    h, w = 50, 47
    k, img = _camera(h, w), _image(h, w, 4)[None]
    clean, holes = _depth(h, w, 5, holes=False)[None], _depth(h, w, 6)[None]
    n, m = _check_mesh(ops, clean, img, k, edge_thr=0.0)  # every pixel kept, every edge joined: two faces per cell
    assert n[0] == h * w and m[0] == 2 * (h - 1) * (w - 1)
    for stride in (2, 4):
        gh, gw = math.ceil(h / stride), math.ceil(w / stride)
        n, m = _check_mesh(ops, clean, img, k, edge_thr=0.0, stride=stride)
        assert n[0] == gh * gw and m[0] == 2 * (gh - 1) * (gw - 1)
        _check_mesh(ops, holes, img, k, edge_thr=0.0, stride=stride)
        _check_mesh(ops, holes, img, k, stride=stride)  # filter on: full-resolution neighbours, joined edges at the stride
    nothing = np.full((1, h, w), np.nan, dtype=F32)
    assert _check_mesh(ops, nothing, img, k)[1][0] == 0
    lo, hi = float(np.percentile(clean, 20)), float(np.percentile(clean, 80))
    _check_mesh(ops, clean, img, k, depth_range=(lo, hi))


def test_two_frame_batch_with_different_counts(ops):
    h, w = 45, 67  # 2904 cells: two runs per frame
    d = np.stack([_depth(h, w, 1), _depth(h, w, 2)])
    d[1, 10:30] = np.nan
    img = np.stack([_image(20, 31, 1), _image(20, 31, 2)])
    n, m = _check_mesh(ops, d, img, _camera(h, w))
    assert n[0] != n[1] and m[0] != m[1] and m.min() > 0
    # a frame of a batch equals the frame alone
    _, _, one, m1 = ops.mesh_pack(torch.from_numpy(d[1]).to(DEV), torch.from_numpy(img[1]).to(DEV), _camera(h, w))
    _, _, two, m2 = ops.mesh_pack(torch.from_numpy(d).to(DEV), torch.from_numpy(img).to(DEV), _camera(h, w))
    assert int(m1[0]) == int(m2[1]) and torch.equal(one[0, :13 * int(m1[0])], two[1, :13 * int(m1[0])])


@pytest.mark.parametrize("shape", [(480, 640), (600, 900)])
def test_many_runs(ops, shape):
    """480 x 640: 306081 cells = 150 runs.  600 x 900: 538501 cells = 263 runs (and 264 runs of pixels for the index map), past the
    256 lanes of the one-block scan: a lane's chunk of run counts is two entries long there, one at the smaller shape"""
    h, w = shape
    assert (math.ceil((h - 1) * (w - 1) / RUN) > 256) == (shape == (600, 900))
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    d = (4.0 + 0.8 * np.sin(x / 41.0) * np.cos(y / 29.0) + 0.002 * x + 0.001 * np.random.RandomState(9).rand(h, w)).astype(F32)
    d[200:203, 100:400] = np.nan
    d[:, 500:] += F32(2.0)
    n, m = _check_mesh(ops, d[None], _image(h // 4, w // 4, 9)[None], _camera(h, w))
    assert 0 < m[0] < 2 * (h - 1) * (w - 1)


def test_determinism_and_validation(ops):
    h, w = 61, 83
    d, img, k = torch.from_numpy(_depth(h, w, 8)[None]).to(DEV), torch.from_numpy(_image(40, 50, 8)[None]).to(DEV), _camera(h, w)
    fb = 26 * (h - 1) * (w - 1)
    zeros = lambda nb: torch.zeros((1, nb), dtype=torch.uint8, device=DEV)  # noqa: E731  (the bytes behind the records are not written)
    a = ops.mesh_pack(d, img, k, out_vertices=zeros(15 * h * w), out_faces=zeros(fb))
    b = ops.mesh_pack(d, img, k, out_vertices=zeros(15 * h * w), out_faces=zeros(fb))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for bad in (dict(stride=0), dict(edge_thr=float("nan")), dict(depth_range=(float("nan"), 1.0)),
                dict(out_faces=torch.zeros((1, fb - 1), dtype=torch.uint8, device=DEV)),
                dict(out_vertices=torch.zeros((1, 15 * h * w - 1), dtype=torch.uint8, device=DEV)),
                dict(out_faces=torch.zeros((1, fb), dtype=torch.uint8))):
        with pytest.raises(ValueError):
            ops.mesh_pack(d, img, k, **bad)
    with pytest.raises(ValueError):
        ops.mesh_pack(d, img.cpu(), k)
    with pytest.raises(ValueError):
        ops.mesh_pack(d, torch.ones(2, 3, 4, 5, device=DEV), k)


# ------------------------------------------------------------------------------------------------------------------ OutputStage
def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


@pytest.mark.parametrize("device_deflate", [False, True])
@pytest.mark.parametrize("ply", [False, True])
def test_output_stage_writes_the_host_routes_mesh(tmp_path, ply, device_deflate):
    from patchrefinerv2_amd.output import OutputStage, mesh_faces_host, pointcloud_host, write_geometry_host
    h, w = 61, 83
    d, img, k = _depth(h, w, 11), _image(30, 41, 11), _camera(h, w)
    geo = dict(depth_range=(0.0, float("inf")), edge_thr=0.05, stride=2)
    (tmp_path / "host").mkdir()
    write_geometry_host(str(tmp_path / "host" / "f"), d, img, k, ply=ply, normals=False, mesh=True, **geo)
    host = _files(tmp_path / "host")
    assert set(host) == {"f_mesh.ply"} | ({"f.ply"} if ply else set())
    n, m = pointcloud_host(d, img, k, **geo).size, mesh_faces_host(d, **geo).shape[0]
    assert n > 0 and m > 0

    def run(work, mesh):
        stage = OutputStage(str(tmp_path / work), workers=2, device_deflate=device_deflate)
        stage.submit_geometry(os.path.join(str(tmp_path / work), "f"), torch.from_numpy(d).to(DEV), torch.from_numpy(img), k, ply=ply,
                              normals=False, mesh=mesh, **geo)
        stage.close()
        return _files(tmp_path / work), stage

    dev, stage = run("dev", True)
    assert dev == host
    off, stage_off = run("off", False)
    assert off == {n: v for n, v in host.items() if n != "f_mesh.ply"}  # <name>.ply does not depend on the new flag
    assert stage.bytes_d2h - stage_off.bytes_d2h == 15 * n + 13 * m + 16 and stage.files - stage_off.files == 1


# ------------------------------------------------------------------------------------------------------------------ Tester
def test_tester_run_writes_the_host_routes_mesh(tmp_path):
    """Tester.run --save --device-output --save-ply --save-mesh against the host route (an m-mode: the intrinsics are scaled to the
    re-ensemble shape), and the mesh's share of the copies"""
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
    geo = dict(save_ply=True, fov=70.0, ply_stride=3, ply_edge_thr=0.05, ply_depth_range=(0.0, float("inf")))

    def run(work, **info):
        t = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path / work), output_workers=4, **geo, **info), ds, m)
        t.run(cai_mode="m1", image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621)
        return _files(tmp_path / work), t.last_output_stage

    host, _ = run("host", save_mesh=True)
    dev, stage = run("dev", device_output=True, save_mesh=True)
    off, stage_off = run("off", device_output=True)
    assert set(dev) == set(host) == set(off) | {"f0_mesh.ply"}
    assert dev["f0_mesh.ply"] == host["f0_mesh.ply"] and dev["f0.ply"] == host["f0.ply"] == off["f0.ply"]
    head = dev["f0_mesh.ply"].split(b"end_header\n")[0]
    n, nf = (int(head.split(b"element %s " % e)[1].split(b"\n")[0]) for e in (b"vertex", b"face"))
    assert n > 0 and nf > 0 and len(dev["f0_mesh.ply"]) == len(head) + 11 + 15 * n + 13 * nf
    assert stage.files - stage_off.files == 1 and stage.bytes_d2h - stage_off.bytes_d2h == 15 * n + 13 * nf + 16
