"""CPU: the host specification of the novel-view export (patchrefinerv2_amd/output.py: view_source_host / view_image_host /
view_poses), checked on scenes whose views can be written down by hand and against a face-by-face restatement in plain Python;
the host route's files, the tester's options, the CLI's flags, and the C entry points (declared, bound, exported, rejecting bad
arguments without a GPU)."""
import ctypes
import io
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = float("inf")
SYMBOLS = ("prv2_view_max_face", "prv2_view_stages", "prv2_view_workspace_bytes", "prv2_view_source", "prv2_view_rows")
K = (50.0, 55.0, 20.25, 6.5)


def _pose(tx=0.0, ty=0.0, tz=0.0, yaw=0.0):
    """[R | t] with R a rotation about y by ``yaw`` radians"""
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([c, 0, s, tx, 0, 1, 0, ty, -s, 0, c, tz], dtype=np.float64).astype(F32)


def _image(hi, wi, seed):
    img = np.random.RandomState(100 + seed).rand(3, hi, wi).astype(F32) * F32(1.2) - F32(0.1)
    img.reshape(-1)[::31] = np.nan
    return img


def _bytes(img):
    from patchrefinerv2_amd.output import color_bytes
    with np.errstate(all="ignore"):
        return np.moveaxis(color_bytes(img * F32(255)), 0, -1)


def _decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


# ---------------------------------------------------------------------------------------------- a restatement in plain Python
def _restated(d, k, pose, depth_range=(0.0, INF), edge_thr=0.05, max_face=16):
    """include/prv2.h "Novel-view export" one vertex, one face and one pixel at a time, with numpy float32 scalars"""
    h, w = d.shape
    fx, fy, cx, cy = (F32(v) for v in k)
    M = [F32(v) for v in pose]
    lo, hi, thr = F32(depth_range[0]), F32(depth_range[1]), F32(edge_thr)
    valid, vert = {}, {}
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                Z = d[y, x]
                valid[y, x] = bool(np.isfinite(Z) and lo < Z < hi)
                vert[y, x] = None
                if not valid[y, x]:
                    continue
                X, Y = ((F32(x) + F32(0.5)) - cx) * Z / fx, ((F32(y) + F32(0.5)) - cy) * Z / fy
                Xc, Yc, Zc = (((M[4 * r] * X + M[4 * r + 1] * Y) + M[4 * r + 2] * Z) + M[4 * r + 3] for r in range(3))
                iz = F32(1) / Zc
                fu, fv = fx * (Xc / Zc) + cx, fy * (Yc / Zc) + cy
                if np.isfinite(Zc) and Zc > 0 and np.isfinite(iz) and abs(fu) < 65536 and abs(fv) < 65536:
                    vert[y, x] = (int(np.rint(fu * F32(16))), int(np.rint(fv * F32(16))), iz, y * w + x)
    best = {}

    def offer(px, py, q, source):
        key = ((0xFFFFFFFF - int(np.asarray(q, dtype=F32).view(np.uint32))) << 32) | source
        if 0 <= px < w and 0 <= py < h and key < best.get((py, px), 1 << 64):
            best[py, px] = key

    def joined(p, q):
        if not (valid[p] and valid[q]):
            return False
        with np.errstate(all="ignore"):
            return not thr > 0 or not abs(d[p] - d[q]) > thr * min(d[p], d[q])

    for v in vert.values():
        if v is not None:
            offer(v[0] >> 4, v[1] >> 4, v[2], v[3])
    for y in range(h - 1):
        for x in range(w - 1):
            a, b, c, e = (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1)
            kept = [valid[p] for p in (a, b, c, e)]
            if sum(kept) < 3:
                continue
            ad = abs(d[a] - d[e]) <= abs(d[b] - d[c]) if all(kept) else valid[a] and valid[e]
            for tri in ((a, c, e), (a, e, b)) if ad else ((a, c, b), (b, c, e)):
                p0, p1, p2 = tri
                if not (joined(p0, p1) and joined(p1, p2) and joined(p0, p2)) or any(vert[p] is None for p in tri):
                    continue
                (x0, y0, i0, s0), (x1, y1, i1, s1), (x2, y2, i2, s2) = (vert[p] for p in tri)
                A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
                if A == 0:
                    continue
                s = 1 if A > 0 else -1
                bx0, bx1 = -((8 - min(x0, x1, x2)) // 16), (max(x0, x1, x2) - 8) // 16  # ceil, floor
                by0, by1 = -((8 - min(y0, y1, y2)) // 16), (max(y0, y1, y2) - 8) // 16
                if bx1 - bx0 + 1 > max_face or by1 - by0 + 1 > max_face:
                    continue
                for py in range(max(by0, 0), min(by1, h - 1) + 1):
                    for px in range(max(bx0, 0), min(bx1, w - 1) + 1):
                        cx16, cy16 = 16 * px + 8, 16 * py + 8
                        w0 = s * ((x2 - x1) * (cy16 - y1) - (y2 - y1) * (cx16 - x1))
                        w1 = s * ((x0 - x2) * (cy16 - y2) - (y0 - y2) * (cx16 - x2))
                        w2 = s * ((x1 - x0) * (cy16 - y0) - (y1 - y0) * (cx16 - x0))
                        if min(w0, w1, w2) < 0:
                            continue
                        assert w0 + w1 + w2 == abs(A) < 1 << 24
                        q = ((F32(w0) * i0 + F32(w1) * i1) + F32(w2) * i2) / F32(abs(A))
                        offer(px, py, q, (s0, s1, s2)[max(range(3), key=lambda i: ((w0, w1, w2)[i], -i))])
    src, iz = np.full((h, w), -1, np.int32), np.zeros((h, w), F32)
    far = np.zeros((h, w), np.int64)
    for (py, px), key in best.items():
        src[py, px], far[py, px] = key & 0xFFFFFFFF, key >> 32
        iz[py, px] = np.array(0xFFFFFFFF - (key >> 32), dtype=np.uint32).view(F32)
    filled = src.copy()
    for y in range(h):
        shown = [x for x in range(w) if src[y, x] >= 0]
        for x in range(w):
            if src[y, x] >= 0 or not shown:
                continue
            left, right = [q for q in shown if q < x], [q for q in shown if q > x]
            if left and right:
                filled[y, x] = src[y, right[0]] if far[y, right[0]] > far[y, left[-1]] else src[y, left[-1]]
            else:
                filled[y, x] = src[y, right[0]] if right else src[y, left[-1]]
    return src, filled, iz


def _random_scene(h, w, seed, invalid=0.05):
    rs = np.random.RandomState(seed)
    d = (1.0 + 3.0 * rs.rand(h, w)).astype(F32)
    d[rs.rand(h, w) < invalid] = np.nan
    return d


@pytest.mark.parametrize("pose", [_pose(), _pose(tx=-0.11, ty=0.04), _pose(tz=-0.6), _pose(tx=0.3, yaw=0.2), _pose(yaw=1.3)],
                         ids=["identity", "shift", "dolly", "turn", "behind"])
@pytest.mark.parametrize("edge_thr", [0.3, 0.0])
def test_the_vectorised_specification_equals_the_restatement(pose, edge_thr):
    from patchrefinerv2_amd.output import view_source_host
    d = _random_scene(9, 14, 5, invalid=0.1)
    d[2, 3], d[4, 4], d[5, 9] = np.inf, -1.0, 0.0
    for rng in ((0.0, INF), (1.2, 3.7)):
        got = view_source_host(d, K, pose, rng, edge_thr)
        want = _restated(d, K, pose, rng, edge_thr)
        for g, w_, name in zip(got, want, ("src", "filled", "iz")):
            assert g.dtype == w_.dtype and np.array_equal(g.view(np.int32), w_.view(np.int32)), (name, int((g != w_).sum()))
    got, want = view_source_host(d, K, pose, max_face=3), _restated(d, K, pose, max_face=3)
    assert all(np.array_equal(g.view(np.int32), w_.view(np.int32)) for g, w_ in zip(got, want))


# ---------------------------------------------------------------------------------------------- views one can write down
@pytest.mark.parametrize("edge_thr", [0.05, 0.0])
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 7), (17, 66), (33, 130)], ids=lambda s: "x".join(map(str, s)))
def test_the_identity_pose_shows_every_valid_pixel_as_itself(shape, edge_thr):
    from patchrefinerv2_amd.output import IDENTITY_POSE, view_image_host, view_poses, view_source_host
    h, w = shape
    d = _random_scene(h, w, h * 100 + w)
    k = (40.0, 43.0, w / 2 + 0.3, h / 2 - 0.2)
    src, filled, iz = view_source_host(d, k, IDENTITY_POSE, edge_thr=edge_thr)
    valid = np.isfinite(d)
    index = np.arange(h * w).reshape(h, w)
    assert src.dtype == filled.dtype == np.int32 and iz.dtype == F32
    assert np.array_equal(src, np.where(valid, index, -1))
    assert np.array_equal(iz[valid], (F32(1) / d[valid]).astype(F32)) and not iz[~valid].any()
    assert np.array_equal(filled[valid], index[valid])
    assert ((filled >= 0).all(axis=1) == valid.any(axis=1)).all() and ((filled < 0).all(axis=1) == ~valid.any(axis=1)).all()
    img = _image(h + 2, 2 * w + 1, 3)
    from patchrefinerv2_amd.output import _sampled_bytes
    want = _sampled_bytes(img, h, w, np.arange(h)[:, None], np.arange(w)[None, :])
    got = view_image_host(d, img, k, IDENTITY_POSE, edge_thr=edge_thr)
    assert got.dtype == np.uint8 and got.shape == (h, w, 3) and np.array_equal(got[valid], want[valid])
    assert np.array_equal(view_poses(1, amplitude=0.0)[0], np.array(IDENTITY_POSE, dtype=F32))
    # the default pose is the identity
    assert all(np.array_equal(a, b) for a, b in zip(view_source_host(d, k, edge_thr=edge_thr), (src, filled, iz)))


def test_a_plane_shifts_by_whole_columns():
    """Z = 2, fx = 64, the eye 0.125 m to the right: every row is the image 4 columns to the left; the 4 columns at the right edge
    are holes, filled from the one side that exists"""
    from patchrefinerv2_amd.output import view_image_host, view_source_host
    h, w = 9, 40
    d = np.full((h, w), 2.0, dtype=F32)
    k = (64.0, 64.0, 20.0, 4.5)
    src, filled, iz = view_source_host(d, k, _pose(tx=-0.125))
    index = np.arange(h * w).reshape(h, w)
    assert np.array_equal(src[:, :w - 4], index[:, 4:]) and (src[:, w - 4:] == -1).all()
    assert np.array_equal(filled[:, :w - 4], index[:, 4:]) and np.array_equal(filled[:, w - 4:], np.repeat(index[:, -1:], 4, axis=1))
    assert (iz[:, :w - 4] == F32(0.5)).all() and not iz[:, w - 4:].any()
    img = _image(h, w, 1)
    view = view_image_host(d, img, k, _pose(tx=-0.125))
    assert np.array_equal(view[:, :w - 4], _bytes(img)[:, 4:]) and np.array_equal(view[:, w - 4:], np.repeat(_bytes(img)[:, -1:], 4, axis=1))


def test_a_near_block_occludes_the_wall_and_its_hole_is_filled_from_the_wall():
    from patchrefinerv2_amd.output import view_poses, view_source_host
    h, w = 12, 48
    d = np.full((h, w), 4.0, dtype=F32)
    d[3:9, 16:26] = 1.0
    k = (40.0, 40.0, 24.0, 6.0)
    pose = view_poses(4, "sway", 0.1)[1]  # the eye 0.1 m to the right: the block moves 4 columns to the left, the wall 1
    assert np.allclose(pose, _pose(tx=-0.1))
    src, filled, iz = view_source_host(d, k, pose)
    index = np.arange(h * w).reshape(h, w)
    assert np.array_equal(src[3:9, 12:22], index[3:9, 16:26])             # the block wins where both project
    assert (iz[3:9, 12:22] == F32(1.0)).all()
    assert (src[3:9, 22:25] == -1).all() and (src[3:9, 25] == index[3:9, 26]).all()  # the disocclusion on its right
    assert (d.reshape(-1)[filled[3:9, 22:25]] == 4.0).all()              # filled from the wall's side,
    assert np.array_equal(filled[3:9, 22:25], np.repeat(index[3:9, 26:27], 3, axis=1))  # its nearest shown column
    assert np.array_equal(src[0, :w - 1], index[0, 1:]) and (iz[0, :w - 1] == F32(0.25)).all()
    want = _restated(d, k, pose)
    assert all(np.array_equal(g.view(np.int32), w_.view(np.int32)) for g, w_ in zip((src, filled, iz), want))


def test_the_cap_drops_faces_stretched_more_than_sixteen_fold():
    from patchrefinerv2_amd.output import VIEW_MAX_FACE, _view_vertices, view_source_host
    h, w = 21, 31
    d = np.full((h, w), 3.0, dtype=F32)
    k = (30.0, 30.0, 15.5, 10.5)  # the middle pixel's centre is the principal point
    assert VIEW_MAX_FACE == 16
    src3, filled3, _ = view_source_host(d, k, _pose(tz=-2.0))  # Zc = 1: magnified 3-fold
    assert (src3 >= 0).all() and np.array_equal(src3, filled3)
    assert src3[10, 15] == 10 * w + 15 and (np.abs(src3 // w - 10) <= 4).all() and (np.abs(src3 % w - 15) <= 6).all()
    pose40 = _pose(tz=-(3.0 - 3.0 / 40.0))
    src40, filled40, _ = view_source_host(d, k, pose40)
    assert (src40 == -1).any() and (src40 >= 0).any() and (filled40[(src40 >= 0).any(axis=1)] >= 0).all()
    _, seen, ux, uy, _ = _view_vertices(d, k, pose40, (0.0, INF))
    ys, xs = np.nonzero(src40 >= 0)
    for y, x in zip(ys, xs):  # only the point candidates remain: a shown pixel holds the vertex that falls into it
        sy, sx = divmod(int(src40[y, x]), w)
        assert seen[sy, sx] and (ux[sy, sx] >> 4, uy[sy, sx] >> 4) == (x, y)
    assert (view_source_host(d, k, pose40, max_face=64)[0] >= 0).all()  # with a cap past the stretch the plane is closed again


def test_what_lies_behind_the_camera_is_not_shown():
    from patchrefinerv2_amd.output import _view_vertices, view_image_host, view_source_host
    h, w = 10, 40
    d = _random_scene(h, w, 9, invalid=0.0)
    k = (12.0, 12.0, 20.0, 5.0)
    pose = _pose(yaw=1.2)
    with np.errstate(all="raise"):
        src, filled, iz = view_source_host(d, k, pose)
        view_image_host(d, _image(h, w, 0), k, pose)
    _, seen, _, _, _ = _view_vertices(d, k, pose, (0.0, INF))
    X = ((np.arange(w, dtype=F32) + F32(0.5)) - F32(20.0))[None, :] * d / F32(12.0)
    zc = -math.sin(1.2) * X.astype(np.float64) + math.cos(1.2) * d
    assert (zc < -0.01).any() and (zc > 0.01).any() and not seen[zc < -0.01].any()
    assert seen.reshape(-1)[src[src >= 0]].all()
    assert all(np.array_equal(g.view(np.int32), w_.view(np.int32)) for g, w_ in zip((src, filled, iz), _restated(d, k, pose)))


# ---------------------------------------------------------------------------------------------- the camera path
def test_view_poses():
    from patchrefinerv2_amd.output import IDENTITY_POSE, view_poses
    p = view_poses(8, "circle", 0.05)
    assert p.dtype == F32 and p.shape == (8, 12)
    R, t = p.reshape(8, 3, 4)[:, :, :3], p.reshape(8, 3, 4)[:, :, 3]
    assert (R == np.eye(3, dtype=F32)).all()  # focus = inf: the identity exactly
    assert np.array_equal(t[0], np.array([-0.05, 0, 0], dtype=F32))  # the first eye at (A, 0, 0): t = -e
    assert np.allclose(t[2], [0, -0.05, 0], atol=1e-9) and np.allclose(t[4], [0.05, 0, 0], atol=1e-9)
    assert np.array_equal(view_poses(1, "sway", 0.3)[0], np.array(IDENTITY_POSE, dtype=F32))
    assert np.allclose(view_poses(4, "sway", 0.2).reshape(4, 3, 4)[:, :, 3], [[0, 0, 0], [-0.2, 0, 0], [0, 0, 0], [0.2, 0, 0]], atol=1e-9)
    assert np.allclose(view_poses(4, "dolly", 0.2).reshape(4, 3, 4)[:, :, 3], [[0, 0, 0], [0, 0, -0.2], [0, 0, 0], [0, 0, 0.2]], atol=1e-9)
    assert (view_poses(5, "circle", 0.0, 2.0) == np.array(IDENTITY_POSE, dtype=F32)).all()
    for motion in ("circle", "sway", "dolly"):
        for k in range(7):
            th = 2 * math.pi * k / 7
            e = 0.3 * np.array({"circle": (math.cos(th), math.sin(th), 0), "sway": (math.sin(th), 0, 0), "dolly": (0, 0, math.sin(th))}[motion])
            M = view_poses(7, motion, 0.3, 2.5)[k].astype(np.float64).reshape(3, 4)
            assert np.allclose(M[:, :3] @ M[:, :3].T, np.eye(3), atol=1e-6) and np.linalg.det(M[:, :3]) > 0.99
            assert np.allclose(M[:, :3] @ e + M[:, 3], 0, atol=1e-6)  # the eye is the new origin
    # a finite focus keeps (0, 0, focus) on the principal point: to 1e-6 px in float64 (before the one rounding)
    fx, focus, A = 2000.0, 2.5, 0.3
    for k in range(7):
        th = 2 * math.pi * k / 7
        e = A * np.array((math.cos(th), math.sin(th), 0.0))
        f = np.array((0, 0, focus)) - e
        f /= np.linalg.norm(f)
        r = np.cross((0, 1, 0), f)
        r /= np.linalg.norm(r)
        R64 = np.stack([r, np.cross(f, r), f])
        c = R64 @ (np.array((0, 0, focus)) - e)
        assert abs(fx * c[0] / c[2]) < 1e-6 and abs(fx * c[1] / c[2]) < 1e-6 and c[2] > 0
        assert np.array_equal(view_poses(7, "circle", A, focus)[k], np.concatenate([R64, -(R64 @ e)[:, None]], axis=1).reshape(12).astype(F32))
    for bad in (dict(count=0), dict(count=121), dict(count=4, motion="orbit"), dict(count=4, amplitude=-0.1), dict(count=4, amplitude=INF),
                dict(count=4, amplitude=float("nan")), dict(count=4, focus=0.0), dict(count=4, focus=-1.0), dict(count=4, focus=float("nan"))):
        with pytest.raises(ValueError):
            view_poses(**bad)


# ---------------------------------------------------------------------------------------------- host route, tester, CLI
def test_host_route_files_and_tester_options(tmp_path):
    from patchrefinerv2_amd import output as O
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    d = torch.from_numpy(_random_scene(24, 40, 3, invalid=0.0))[None, None]
    img = torch.from_numpy(_image(24, 40, 1))
    item = dict(img_file_basename="f", image_hr=img[None])
    k = O.camera_intrinsics((24, 40), (24, 40), fov=70.0)

    def files(work):
        return {n: (tmp_path / work / n).read_bytes() for n in sorted(os.listdir(tmp_path / work))}

    views = dict(count=3, motion="circle", amplitude=0.2, focus=3.0)
    for work, kw in (("g0", {}), ("g1", dict(views=None)), ("g2", dict(views=views))):
        (tmp_path / work).mkdir()
        O.write_geometry_host(str(tmp_path / work / "f"), d[0, 0].numpy(), img.numpy(), k, ply=False, **kw)
    names = {"f_view_000.png", "f_view_001.png", "f_view_002.png"}
    assert set(files("g0")) == {"f_normal.png"} and files("g1") == files("g0") and set(files("g2")) == names | {"f_normal.png"}
    poses = O.view_poses(**views)
    for i in range(3):
        assert np.array_equal(_decode(files("g2")[f"f_view_{i:03d}.png"]), O.view_image_host(d[0, 0].numpy(), img.numpy(), k, poses[i]))
    assert not np.array_equal(_decode(files("g2")["f_view_000.png"]), _decode(files("g2")["f_view_001.png"]))
    for bad in (dict(number=3), dict(count=0), dict(count=3, motion="orbit"), dict(count=3, focus=0.0)):
        with pytest.raises(ValueError):
            O.write_geometry_host(str(tmp_path / "g0" / "x"), d[0, 0].numpy(), img.numpy(), k, ply=False, normals=False, views=bad)
    assert O._view_options(dict(count=5)) == dict(count=5, motion="circle", amplitude=0.05, focus=INF)

    for flags in (dict(), dict(save_views=0)):
        assert Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path), **flags), None, None)._geometry(d, (24, 40)) is None
    assert Tester(None, RunnerInfo(save=False, work_dir=str(tmp_path), save_views=3), None, None)._geometry(d, (24, 40)) is None
    geo = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path), save_views=3), None, None)._geometry(d, (24, 40))
    assert geo["views"] == dict(count=3, motion="circle", amplitude=0.05, focus=INF) and not (geo["ply"] or geo["normals"] or geo["mesh"])
    assert "views" not in Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path), save_ply=True), None, None)._geometry(d, (24, 40))

    def run(work, **flags):
        info = RunnerInfo(save=True, work_dir=str(tmp_path / work), fov=70.0, ply_edge_thr=0.3, ply_depth_range=(0.0, 9.0), **flags)
        Tester(None, info, None, None)._emit([], item, d, None, (24, 40))
        return files(work)

    plain = run("plain")
    assert set(plain) == {"f.png", "f_uint16.png", "f_edge.png"} and run("off", save_views=0) == plain
    two = run("two", save_views=2, view_motion="dolly", view_amplitude=0.5, view_focus=4.0)
    assert set(two) == set(plain) | {"f_view_000.png", "f_view_001.png"} and {n: v for n, v in two.items() if "_view_" not in n} == plain
    poses = O.view_poses(2, "dolly", 0.5, 4.0)
    for i in range(2):
        want = O.view_image_host(d[0, 0].numpy(), img.numpy(), k, poses[i], (0.0, 9.0), 0.3)
        assert np.array_equal(_decode(two[f"f_view_{i:03d}.png"]), want)


@pytest.mark.parametrize("flags,message", [
    (["--save-views", "4"], "need --save"),
    (["--save-views", "4", "--view-motion", "sway", "--view-amplitude", "0.1", "--view-focus", "2"], "need --save"),
    (["--save", "--save-views", "121"], "--save-views"),
    (["--save", "--save-views", "-1"], "--save-views"),
    (["--save", "--save-views", "4", "--view-motion", "orbit"], "--view-motion"),
    (["--save", "--save-views", "4", "--view-amplitude", "-1"], "--view-amplitude"),
    (["--save", "--save-views", "4", "--view-focus", "0"], "--view-focus"),
])
def test_cli_argument_errors(flags, message):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "no_such_config.py", *flags], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]


def test_cli_help_names_the_flags_and_the_host_routes_cost():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    text = " ".join(r.stdout.split())
    assert r.returncode == 0 and all(f in text for f in ("--save-views", "--view-motion", "--view-amplitude", "--view-focus"))
    assert "not a route for 4K" in text


# ---------------------------------------------------------------------------------------------- the C ABI
def _arg_count(hdr, name):
    args = re.search(rf"\b{name}\s*\(([^)]*)\)", hdr).group(1)
    return 0 if args.strip() in ("", "void") else len(args.split(","))


def test_entry_points_declared_bound_exported_and_ops_registered():
    from patchrefinerv2_amd import lib as L, ops, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20 and "Novel-view export" in hdr
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.SIGNATURES and hasattr(raw, name), name
        assert _arg_count(hdr, name) == len(L.SIGNATURES[name][1]), name
    lib = L.load()
    assert lib.prv2_abi_version() == 20 and lib.prv2_view_max_face() == 16 == ops.view_max_face()
    assert lib.prv2_view_workspace_bytes(2, 3, 5, 7) == 8 * 2 * 3 * 5 * 7
    assert lib.prv2_view_workspace_bytes(1, 4, 2160, 3840) == 8 * 4 * 2160 * 3840
    for bad in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (1, 1, 1 << 15, 1 << 14), (1, 64, 4096, 2048), (64, 1, 4096, 2048)):
        assert lib.prv2_view_workspace_bytes(*bad) == -1, bad
    t = torch_ops.load()
    for name in ("view_source", "view_rows"):
        assert name in torch_ops.OPS and hasattr(ops, name)
        getattr(t, name).default._schema
    with pytest.raises((NotImplementedError, RuntimeError)):
        t.view_source(torch.zeros(1, 4, 4), [5.0, 5.0, 2.0, 2.0], torch.zeros(1, 12), 0.0, INF, 0.05)  # no CPU implementation to fall into


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    err = lambda: lib.prv2_last_error().decode()  # noqa: E731
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4104)  # never dereferenced: every call fails its argument check before a launch
    limit = lib.prv2_stereo_max_width()

    def source(depth=p, n=1, h=4, w=4, fx=5.0, cy=2.0, poses=p, nv=2, lo=0.0, thr=0.05, src=p, filled=p, iz=p, ws=p, nbytes=8 * 2 * 16):
        return lib.prv2_view_source(depth, n, h, w, fx, 5.0, 2.0, cy, poses, nv, lo, INF, thr, src, filled, iz, ws, nbytes, None)
    assert source(depth=None) != 0 and "null" in err()
    assert source(poses=None) != 0 and "null" in err()
    assert source(src=None) != 0 and "null" in err()
    assert source(filled=None) != 0 and "null" in err()
    assert source(n=0) != 0 and "frame count" in err()
    assert source(h=0) != 0 and "shape" in err()
    assert source(nv=0) != 0 and "view count" in err()
    assert source(h=4096, w=4096, nv=32, nbytes=1 << 40) != 0 and "2^29" in err()
    assert source(w=limit + 1, nbytes=1 << 40) != 0 and str(limit) in err() and "prv2_stereo_max_width" in err()
    assert source(fx=0.0) != 0 and "intrinsics" in err()
    assert source(cy=INF) != 0 and "intrinsics" in err()
    assert source(lo=float("nan")) != 0 and "NaN" in err()
    assert source(thr=float("nan")) != 0 and "NaN" in err()
    assert source(ws=None) != 0 and "workspace" in err()
    assert source(ws=odd) != 0 and "aligned" in err()
    assert source(nbytes=8 * 2 * 16 - 8) != 0 and "prv2_view_workspace_bytes" in err()

    rb = lib.prv2_rows_bytes(4, 4, 3)

    def rows(image=p, ih=8, out=p, vstride=rb, ws=p, nbytes=8 * 2 * 16):
        return lib.prv2_view_rows(p, image, 1, 4, 4, ih, 8, 5.0, 5.0, 2.0, 2.0, p, 2, 0.0, INF, 0.05, out, vstride, ws, nbytes, None)
    assert rows(image=None) != 0 and "null" in err()
    assert rows(ih=0) != 0 and "image shape" in err()
    assert rows(out=None) != 0 and "null" in err()
    assert rows(out=odd) != 0 and "aligned" in err()
    assert rows(vstride=rb - 16) != 0 and "stride" in err()
    assert rows(vstride=rb + 8) != 0 and "stride" in err()
    assert rows(nbytes=0) != 0 and "workspace" in err()
    with pytest.raises(RuntimeError):
        L.check(rows(out=None), "view_rows")


def test_wrappers_validate_before_touching_the_gpu():
    from patchrefinerv2_amd import ops
    d = torch.zeros(1, 4, 4)
    with pytest.raises(ValueError, match="GPU"):
        ops.view_source(d, K, np.zeros((1, 12), F32))  # a CPU tensor
    with pytest.raises(ValueError, match="GPU"):
        ops.view_rows(d, torch.zeros(3, 4, 4), K, np.zeros((1, 12), F32))
