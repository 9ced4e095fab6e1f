"""CPU: the host half of the geometry export (patchrefinerv2_amd/output.py).  The host specification of the point cloud and the
normal map against closed forms, the PLY container, the camera from --fov / --intrinsics, the CLI's argument errors, and the C
entry points: declared, bound, exported, and rejecting bad arguments without a GPU."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prv2_pointcloud_count", "prv2_pointcloud_pack", "prv2_normal_rows")
F32 = np.float32
K = np.array([50.0, 55.0, 19.5, 14.25], dtype=F32)  # fx, fy, cx, cy


def _image(h, w, seed=0):
    return np.random.RandomState(seed).rand(3, h, w).astype(F32)


def test_fronto_parallel_plane_points_and_normals():
    from patchrefinerv2_amd import output as O
    h, w, c = 30, 40, F32(2.5)
    d = np.full((h, w), c, dtype=F32)
    v = O.pointcloud_host(d, _image(h, w), K, edge_thr=0.05)
    assert v.dtype == O.PLY_VERTEX and v.dtype.itemsize == 15 and v.size == h * w
    ys, xs = np.divmod(np.arange(h * w), w)
    want_x = ((xs.astype(F32) + F32(0.5)) - K[2]) * c / K[0]
    want_y = ((ys.astype(F32) + F32(0.5)) - K[3]) * c / K[1]
    assert want_x.dtype == F32 and np.array_equal(v["x"], want_x) and np.array_equal(v["y"], want_y) and np.all(v["z"] == c)
    n = O.normal_map_host(d, K)
    assert n.shape == (h, w, 3) and n.dtype == np.uint8
    assert np.all(n == np.array([128, 128, 0], dtype=np.uint8))  # (0, 0, -1): 127.5 rounds to the even 128


def test_tilted_plane_normal_within_one_of_the_analytic_encoding():
    """world plane n . P = d seen by the camera: Z at a pixel = d / (n . ray), ray = (u / fx, v / fy, 1).  fp32 error of the
    normal is ~1e-5, far below 1 / 255, so a byte can differ from the analytic encoding only across a .5 tie: at most by 1"""
    from patchrefinerv2_amd import output as O
    h, w = 30, 40
    nrm = np.array([0.3, -0.2, -0.933], dtype=np.float64)
    nrm /= np.linalg.norm(nrm)
    u = (np.arange(w) + 0.5 - float(K[2])) / float(K[0])
    v = (np.arange(h) + 0.5 - float(K[3])) / float(K[1])
    z = (-4.0 / (nrm[0] * u[None, :] + nrm[1] * v[:, None] + nrm[2])).astype(F32)
    assert (z > 0).all()
    got = O.normal_map_host(z, K).astype(np.int64)
    want = np.rint((nrm * 0.5 + 0.5) * 255)  # faces the camera already: n . P = -4 < 0
    assert np.abs(got - want[None, None, :]).max() <= 1
    # Z = a x + b y + c in pixel coordinates: P(x, y) = (u Z / fx, v Z / fy, Z) is quadratic in x and in y, so the central
    # difference IS twice the analytic derivative and the interior normals are those of cross(dP/dx, dP/dy), evaluated in float64
    # (the border rows and columns take one-sided differences, which are not the derivative)
    a, b, c = 0.01, 0.02, 3.0
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    z2 = a * xx + b * yy + c
    uu, vv = xx + 0.5 - float(K[2]), yy + 0.5 - float(K[3])
    px = np.stack([(z2 + uu * a) / float(K[0]), vv * a / float(K[1]), np.full_like(z2, a)])
    py = np.stack([uu * b / float(K[0]), (z2 + vv * b) / float(K[1]), np.full_like(z2, b)])
    n = np.cross(px, py, axis=0)
    n /= np.linalg.norm(n, axis=0)
    n = np.where((n * np.stack([uu * z2 / float(K[0]), vv * z2 / float(K[1]), z2])).sum(axis=0) > 0, -n, n)
    want2 = np.moveaxis(np.rint((n * 0.5 + 0.5) * 255), 0, -1)
    got2 = O.normal_map_host(z2.astype(F32), K).astype(np.int64)
    assert np.abs(got2 - want2)[1:-1, 1:-1].max() <= 1 and (got2.sum(axis=2) > 0).all()


def test_step_edge_is_dropped_on_both_sides_and_kept_without_the_filter():
    from patchrefinerv2_amd import output as O
    d = np.full((6, 8), 2.0, dtype=F32)
    d[:, 4:] = 3.0  # |3 - 2| = 1 > 0.05 * 2
    keep = O.keep_mask_host(d, edge_thr=0.05)
    want = np.ones((6, 8), dtype=bool)
    want[:, 3:5] = False
    assert np.array_equal(keep, want)
    assert O.keep_mask_host(d, edge_thr=0.0).all() and O.keep_mask_host(d, edge_thr=-1.0).all()
    assert O.keep_mask_host(d, edge_thr=0.6).all()  # 1 > 0.6 * 2 is false
    assert O.pointcloud_host(d, _image(6, 8), K, edge_thr=0.05).size == 6 * 6
    # an invalid neighbour and the frame border do not drop a pixel
    e = np.full((5, 5), 2.0, dtype=F32)
    e[2, 2] = np.nan
    k = O.keep_mask_host(e, edge_thr=0.05)
    assert not k[2, 2] and k.sum() == 24
    # the filter does not apply to the normal map: both sides of the step have normals
    assert (O.normal_map_host(d, K).sum(axis=2) > 0).all()


def test_invalid_depths_and_the_range():
    from patchrefinerv2_amd import output as O
    d = np.full((4, 6), 5.0, dtype=F32)
    d[0, 0], d[0, 1], d[0, 2], d[0, 3], d[0, 4] = np.nan, np.inf, 0.0, -1.0, -np.inf
    keep = O.keep_mask_host(d, edge_thr=0.0)
    assert not keep[0, :5].any() and keep.sum() == 24 - 5
    n = O.normal_map_host(d, K)
    assert not n[0, :5].any() and n[2, 2].any()
    r = np.arange(1, 25, dtype=F32).reshape(4, 6)
    k = O.keep_mask_host(r, depth_range=(3.0, 20.0), edge_thr=0.0)
    assert np.array_equal(k, (r > 3) & (r < 20))  # both ends are open


def test_stride_keeps_the_grid_and_colour_indices_follow_the_integer_formula():
    from patchrefinerv2_amd import output as O
    h, w, hi, wi = 30, 40, 45, 70
    d = np.full((h, w), 1.5, dtype=F32)
    keep = O.keep_mask_host(d, edge_thr=0.0, stride=3)
    ys, xs = np.nonzero(keep)
    assert np.all(ys % 3 == 0) and np.all(xs % 3 == 0) and keep.sum() == 10 * 14
    with pytest.raises(ValueError):
        O.pointcloud_host(d, _image(hi, wi), K, stride=0)
    sy, sx = O.sample_indices(h, hi), O.sample_indices(w, wi)
    assert [int(v) for v in sy] == [((2 * y + 1) * hi) // (2 * h) for y in range(h)]
    assert [int(v) for v in sx] == [((2 * x + 1) * wi) // (2 * w) for x in range(w)]
    assert sy.max() == hi - 1 and sx.max() == wi - 1 and sy.min() == 0
    # an image that codes its own position: the cloud's colours are the formula's samples
    img = np.zeros((3, hi, wi), dtype=F32)
    img[0] = (np.arange(hi, dtype=F32) / F32(255))[:, None]
    img[1] = (np.arange(wi, dtype=F32) / F32(255))[None, :]
    img[2] = 0.5
    v = O.pointcloud_host(d, img, K, edge_thr=0.0)
    ys, xs = np.divmod(np.arange(h * w), w)
    assert np.array_equal(v["red"], sy[ys]) and np.array_equal(v["green"], sx[xs]) and np.all(v["blue"] == 128)
    assert [int(b) for b in O.color_bytes(np.array([0.5, 1.5, 2.5, -3.0, 300.0, np.nan, np.inf, -np.inf], dtype=F32))] == [0, 2, 2, 0, 255, 0, 255, 0]


def test_ply_round_trip_and_empty_cloud():
    from patchrefinerv2_amd import output as O
    rs = np.random.RandomState(5)
    d = (rs.rand(13, 17) * 0.5 + 5).astype(F32)  # neighbours differ by up to 0.5: some exceed 0.05 * 5
    v = O.pointcloud_host(d, _image(20, 11), K, edge_thr=0.05, stride=2)
    assert 0 < v.size < 7 * 9
    for verts in (v, v[:0]):
        data = O.ply_bytes(verts.size, verts.tobytes())
        head, _, body = data.partition(b"end_header\n")
        lines = head.decode("ascii").split("\n")
        assert lines[:3] == ["ply", "format binary_little_endian 1.0", f"element vertex {verts.size}"]
        assert lines[3:] == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
                             "property uchar blue", ""]
        assert len(data) == len(O.ply_header(verts.size)) + 15 * verts.size
        back = np.frombuffer(body, dtype=O.PLY_VERTEX)
        assert back.size == verts.size and back.tobytes() == verts.tobytes()
    # a longer buffer (the device route's bound) is cut at 15 N; a shorter one is an error
    assert O.ply_bytes(2, v.tobytes()) == O.ply_header(2) + v[:2].tobytes()
    with pytest.raises(ValueError):
        O.ply_bytes(v.size + 1, v.tobytes())


def test_intrinsics_from_fov_and_scaled_to_the_result_shape():
    from patchrefinerv2_amd import output as O
    raw = (2160, 3840)
    k = O.camera_intrinsics(raw, raw)  # fov 60
    f = 1920.0 / math.tan(math.radians(30.0))
    assert k.dtype == F32 and np.array_equal(k, np.array([f, f, 1920.0, 1080.0]).astype(F32))
    k90 = O.camera_intrinsics(raw, raw, fov=90.0)
    assert abs(float(k90[0]) - 1920.0) < 1e-3 and k90[0] == k90[1]
    # an m-mode result at the re-ensemble shape: fx, cx by W / W_raw, fy, cy by H / H_raw, in float64, one cast
    res = (1024, 2048)
    ks = O.camera_intrinsics(raw, res, intrinsics=(3000.0, 2900.0, 1900.5, 1100.25))
    want = np.array([3000.0 * (2048 / 3840), 2900.0 * (1024 / 2160), 1900.5 * (2048 / 3840), 1100.25 * (1024 / 2160)]).astype(F32)
    assert np.array_equal(ks, want)
    kf = O.camera_intrinsics(raw, res, fov=60.0)
    assert np.array_equal(kf, np.array([f * (2048 / 3840), f * (1024 / 2160), 1024.0, 512.0]).astype(F32))
    with pytest.raises(ValueError):
        O.camera_intrinsics(raw, raw, fov=180.0)


def test_tester_host_route_writes_the_specification(tmp_path):
    """Tester._emit without a stage: <name>.ply and <name>_normal.png come from the host specification, at the result's grid"""
    from patchrefinerv2_amd import output as O
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    rs = np.random.RandomState(3)
    d = (rs.rand(1, 1, 12, 20) * 5 + 1).astype(F32)
    img = torch.from_numpy(_image(24, 40, 1))
    info = RunnerInfo(save=False, work_dir=str(tmp_path), save_ply=True, save_normals=True)
    t = Tester(None, info, None, None)
    assert t._geometry(torch.from_numpy(d), (24, 40)) is None  # nothing without save
    info.save = True
    info.ply_stride, info.ply_edge_thr, info.fov = 2, 0.3, 70.0
    geo = t._geometry(torch.from_numpy(d), (24, 40))
    k = O.camera_intrinsics((24, 40), (12, 20), fov=70.0)
    assert np.array_equal(geo["intrinsics"], k) and geo["stride"] == 2 and geo["depth_range"] == (0.0, float("inf"))
    O.write_geometry_host(str(tmp_path / "f"), d[0, 0], img.numpy(), geo.pop("intrinsics"), **geo)
    v = O.pointcloud_host(d[0, 0], img.numpy(), k, edge_thr=0.3, stride=2)
    assert (tmp_path / "f.ply").read_bytes() == O.ply_bytes(v.size, v.tobytes())
    O.write_png8(str(tmp_path / "want.png"), O.normal_map_host(d[0, 0], k))
    assert (tmp_path / "f_normal.png").read_bytes() == (tmp_path / "want.png").read_bytes()


@pytest.mark.parametrize("flags,message", [
    (["--save-ply"], "need --save"),
    (["--save-normals"], "need --save"),
    (["--save", "--save-ply", "--ply-stride", "0"], "--ply-stride"),
    (["--save", "--save-ply", "--intrinsics", "1", "1", "1", "1", "--fov", "60"], "--intrinsics and --fov"),
])
def test_cli_argument_errors(flags, message):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "no_such_config.py", *flags], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]


def test_entry_points_declared_bound_exported_and_ops_registered():
    from patchrefinerv2_amd import lib as L, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20 and "Geometry export" in hdr
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS + ("prv2_pointcloud_workspace_bytes", "prv2_pointcloud_bound"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.SIGNATURES and hasattr(raw, name), name
    assert L.load().prv2_abi_version() == 20
    ops = torch_ops.load()
    for name in ("pointcloud_pack", "normal_rows"):
        assert name in torch_ops.OPS
        getattr(ops, name).default._schema
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.normal_rows(torch.zeros(1, 4, 4), [1.0, 1.0, 2.0, 2.0], 0.0, 1.0)  # no CPU implementation to fall into


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    err = lambda: lib.prv2_last_error().decode()  # noqa: E731
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)  # never dereferenced: every call fails its argument check before a launch
    inf = float("inf")
    assert lib.prv2_pointcloud_bound(30, 40, 3) == 15 * 10 * 14 and lib.prv2_pointcloud_bound(30, 40, 0) == -1
    ws = lib.prv2_pointcloud_workspace_bytes(2, 100, 100)
    assert ws == 2 * 4 * 5 and lib.prv2_pointcloud_workspace_bytes(0, 4, 4) == -1  # runs of 2048 pixels: ceil(10000 / 2048) = 5

    def count(depth=p, n=2, h=100, w=100, fx=50.0, cx=1.0, stride=1, counts=p, wsp=p, wsb=ws):
        return lib.prv2_pointcloud_count(depth, n, h, w, fx, 50.0, cx, 1.0, 0.0, inf, 0.05, stride, counts, wsp, wsb, None)
    assert count(depth=None) != 0 and "null" in err()
    assert count(counts=None) != 0 and "null" in err()
    assert count(n=0) != 0 and "frame count" in err()
    assert count(h=0) != 0 and "shape" in err()
    assert count(fx=0.0) != 0 and "focal" in err()
    assert count(cx=float("nan")) != 0 and "principal" in err()
    assert count(stride=0) != 0 and "stride" in err()
    assert count(wsp=None) != 0 and "workspace" in err()
    assert count(wsp=odd) != 0 and "aligned" in err()
    assert count(wsb=ws - 1) != 0 and "workspace" in err()

    bound = lib.prv2_pointcloud_bound(100, 100, 1)

    def pack(image=p, ih=8, verts=p, fstride=bound, stride=1):
        return lib.prv2_pointcloud_pack(p, image, 2, 100, 100, ih, 8, 50.0, 50.0, 1.0, 1.0, 0.0, inf, 0.05, stride, p, ws, verts, fstride, None)
    assert pack(image=None) != 0 and "null" in err()
    assert pack(verts=None) != 0 and "null" in err()
    assert pack(ih=0) != 0 and "image shape" in err()
    assert pack(fstride=bound - 1) != 0 and "stride" in err()
    rb = lib.prv2_rows_bytes(4, 4, 3)
    assert lib.prv2_normal_rows(None, 1, 4, 4, 5.0, 5.0, 2.0, 2.0, 0.0, inf, p, rb, None) != 0 and "null" in err()
    assert lib.prv2_normal_rows(p, 1, 4, 4, -5.0, 5.0, 2.0, 2.0, 0.0, inf, p, rb, None) != 0 and "focal" in err()
    assert lib.prv2_normal_rows(p, 1, 4, 4, 5.0, 5.0, 2.0, 2.0, 0.0, inf, odd, rb, None) != 0 and "aligned" in err()
    assert lib.prv2_normal_rows(p, 1, 4, 4, 5.0, 5.0, 2.0, 2.0, 0.0, inf, p, rb - 16, None) != 0 and "stride" in err()
    with pytest.raises(RuntimeError):
        L.check(lib.prv2_normal_rows(None, 1, 4, 4, 5.0, 5.0, 2.0, 2.0, 0.0, inf, p, rb, None), "normal_rows")


def test_wrappers_validate_before_touching_the_gpu():
    from patchrefinerv2_amd import ops
    with pytest.raises(ValueError, match="intrinsics"):
        ops._camera([1.0, 1.0, 2.0], (0.0, 1.0), "x")
    with pytest.raises(ValueError, match="intrinsics"):
        ops._camera([0.0, 1.0, 2.0, 2.0], (0.0, 1.0), "x")
    with pytest.raises(ValueError, match="NaN"):
        ops._camera([1.0, 1.0, 2.0, 2.0], (float("nan"), 1.0), "x")
    k, (lo, hi) = ops._camera(np.array([0.1, 0.2, 0.3, 0.4]), (0.0, float("inf")), "x")
    assert k == [float(F32(v)) for v in (0.1, 0.2, 0.3, 0.4)] and lo == 0.0 and hi == float("inf")
    d, img, K = torch.zeros(1, 4, 4), torch.zeros(1, 3, 4, 4), [5.0, 5.0, 2.0, 2.0]
    with pytest.raises(ValueError, match="GPU"):  # a host depth map
        ops.pointcloud_pack(d, img, K)
    with pytest.raises(ValueError, match="GPU"):
        ops.normal_rows(d, K)
