"""CPU: the host half of the mesh export (patchrefinerv2_amd/output.py).  The host specification of the faces on hand-checkable
inputs and against a per-cell restatement in plain Python, the PLY container, the C entry points (declared, bound, exported,
rejecting bad arguments without a GPU), the CLI's argument error and the tester's host route."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prv2_mesh_workspace_bytes", "prv2_mesh_bound", "prv2_mesh_index", "prv2_mesh_count", "prv2_mesh_pack")
F32 = np.float32
K = np.array([50.0, 55.0, 19.5, 14.25], dtype=F32)  # fx, fy, cx, cy


def _image(h, w, seed=0):
    return np.random.RandomState(seed).rand(3, h, w).astype(F32)


def _depth(h, w, seed, holes=True):
    """(the recipe of tests/test_geometry_gpu.py) a smooth surface with a step, noise, and every kind of invalid value"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    d = (2.0 + 3.0 * (x > 0.55 * w) + 0.03 * x + 0.02 * y + 0.05 * rs.rand(h, w)).astype(F32)
    if holes and h * w > 8:
        flat = d.reshape(-1)
        idx = rs.choice(h * w, size=max(5, h * w // 23), replace=False)
        flat[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, 0.0, -1.5], dtype=F32), idx.size)
    return d


def _faces_by_cell(depth, depth_range=(0.0, np.inf), edge_thr=0.05, stride=1):
    """the rule of the issue, cell by cell in plain Python (float32 scalars) -> ([M, 3], unjoined edges as a set of index pairs)"""
    from patchrefinerv2_amd.output import keep_mask_host
    d = np.asarray(depth, dtype=F32)
    keep = keep_mask_host(d, depth_range, edge_thr, stride)
    rank = (np.cumsum(keep.reshape(-1)).reshape(keep.shape) - 1)
    node = lambda gy, gx: (int(rank[gy * stride, gx * stride]) if keep[gy * stride, gx * stride] else -1, d[gy * stride, gx * stride])  # noqa: E731
    gh, gw = -(-d.shape[0] // stride), -(-d.shape[1] // stride)
    thr = F32(edge_thr)

    def joined(p, q):
        return not thr > 0 or not (abs(F32(p[1] - q[1])) > F32(thr * min(p[1], q[1])))

    out, cut = [], set()
    for gy in range(gh - 1):
        for gx in range(gw - 1):
            a, b, c, e = node(gy, gx), node(gy, gx + 1), node(gy + 1, gx), node(gy + 1, gx + 1)
            kept = [n for n in (a, b, c, e) if n[0] >= 0]
            for i, p in enumerate(kept):
                for q in kept[i + 1:]:
                    if not joined(p, q):
                        cut.add((min(p[0], q[0]), max(p[0], q[0])))
            if len(kept) < 3:
                continue
            if len(kept) == 4:
                ad = abs(F32(a[1] - e[1])) <= abs(F32(b[1] - c[1]))
            else:
                ad = a[0] >= 0 and e[0] >= 0
            for tri in ((a, c, e), (a, e, b)) if ad else ((a, c, b), (b, c, e)):
                if all(n[0] >= 0 for n in tri) and joined(tri[0], tri[1]) and joined(tri[1], tri[2]) and joined(tri[0], tri[2]):
                    out.append([n[0] for n in tri])
    return np.array(out, dtype="<i4").reshape(-1, 3), cut


def _check_faces(faces, n_vertices, cut):
    """the properties every mesh has: indices in [0, N), no repeated index in a face, no face across an unjoined edge"""
    assert faces.dtype == np.dtype("<i4") and faces.ndim == 2 and faces.shape[1] == 3
    if not faces.size:
        return
    assert faces.min() >= 0 and faces.max() < n_vertices
    assert (faces[:, 0] != faces[:, 1]).all() and (faces[:, 1] != faces[:, 2]).all() and (faces[:, 0] != faces[:, 2]).all()
    for p, q in ((0, 1), (1, 2), (0, 2)):
        lo, hi = np.minimum(faces[:, p], faces[:, q]), np.maximum(faces[:, p], faces[:, q])
        assert not any((int(a), int(b)) in cut for a, b in zip(lo, hi))


def test_two_by_two_and_degenerate_grids():
    from patchrefinerv2_amd import output as O
    f = O.mesh_faces_host(np.full((2, 2), 3.0, dtype=F32))
    assert f.dtype == np.dtype("<i4") and f.tolist() == [[0, 2, 3], [0, 3, 1]]  # the tie |Za - Zd| == |Zb - Zc| takes a-d
    # |Za - Zd| > |Zb - Zc|: the diagonal b-c
    assert O.mesh_faces_host(np.array([[3.0, 3.05], [3.05, 3.12]], dtype=F32)).tolist() == [[0, 2, 1], [1, 2, 3]]
    for shape in ((1, 1), (1, 7), (7, 1)):
        f = O.mesh_faces_host(np.full(shape, 3.0, dtype=F32))
        assert f.shape == (0, 3) and f.dtype == np.dtype("<i4")
    assert O.mesh_faces_host(np.full((3, 3), 3.0, dtype=F32), stride=3).shape == (0, 3)  # one node
    assert O.mesh_faces_host(np.full((5, 5), np.nan, dtype=F32)).shape == (0, 3)
    with pytest.raises(ValueError):
        O.mesh_faces_host(np.full((2, 2), 3.0, dtype=F32), stride=0)


def test_plane_faces_look_at_the_camera():
    from patchrefinerv2_amd import output as O
    d = np.full((3, 3), 2.5, dtype=F32)
    f = O.mesh_faces_host(d)
    assert f.shape == (8, 3)
    v = O.pointcloud_host(d, _image(3, 3), K)
    P = np.stack([v["x"], v["y"], v["z"]], axis=-1).astype(np.float64)
    n = np.cross(P[f[:, 1]] - P[f[:, 0]], P[f[:, 2]] - P[f[:, 0]])
    assert (n[:, 2] < 0).all() and ((n * P[f[:, 0]]).sum(axis=1) < 0).all()
    _check_faces(f, v.size, set())


@pytest.mark.parametrize("corner,want", [("a", [0, 1, 2]), ("b", [0, 1, 2]), ("c", [0, 2, 1]), ("d", [0, 2, 1])])
def test_one_invalid_corner_leaves_the_triangle_of_the_other_three(corner, want):
    """a, d missing: the diagonal b-c; b, c missing: a-d.  Vertex ranks skip the missing corner: without a the kept b, c, d are
    0, 1, 2 and the face is (b, c, d); without b: a, c, d = 0, 1, 2 and (a, c, d); without c: a, b, d = 0, 1, 2 and (a, d, b);
    without d: a, b, c = 0, 1, 2 and (a, c, b)"""
    from patchrefinerv2_amd import output as O
    d = np.full((2, 2), 3.0, dtype=F32)
    d.reshape(-1)["abcd".index(corner)] = np.nan
    assert O.mesh_faces_host(d).tolist() == [want]
    assert _faces_by_cell(d)[0].tolist() == [want]


@pytest.mark.parametrize("case", [dict(), dict(stride=2), dict(stride=4), dict(edge_thr=0.0), dict(edge_thr=0.0, stride=3),
                                  dict(depth_range=(2.5, 6.0))])
def test_specification_equals_the_rule_cell_by_cell(case):
    from patchrefinerv2_amd import output as O
    d = _depth(61, 83, seed=61)
    f = O.mesh_faces_host(d, **case)
    want, cut = _faces_by_cell(d, **case)
    assert f.shape[0] > 100 and np.array_equal(f, want)
    _check_faces(f, int(O.keep_mask_host(d, **case).sum()), cut)
    assert not cut or case.get("edge_thr", 0.05) > 0  # (without the filter every pair is joined)


def test_discontinuity_inside_a_cell_of_four_kept_corners():
    """at a stride the flying-pixel filter (full-resolution neighbours) keeps nodes on both sides of a step: the edges across it
    are not joined, and a cell of four kept corners gives no face or one of two"""
    from patchrefinerv2_amd import output as O
    h, w = 61, 83
    y, x = np.mgrid[0:h, 0:w].astype(F32)
    d = (2.0 + 3.0 * (x >= 47) + 0.03 * x + 0.02 * y + 0.05 * np.random.RandomState(5).rand(h, w)).astype(F32)
    f = O.mesh_faces_host(d, stride=3)
    want, cut = _faces_by_cell(d, stride=3)
    assert np.array_equal(f, want) and cut
    _check_faces(f, int(O.keep_mask_host(d, stride=3).sum()), cut)


def _read_ply(data):
    """a binary little-endian PLY of float x y z + uchar r g b vertices and uchar-int face lists -> (header lines, vertex
    records, [M, 3] faces)"""
    from patchrefinerv2_amd.output import PLY_VERTEX
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == ""
    count = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    n, m = count["vertex"], count["face"]
    assert len(body) == 15 * n + 13 * m
    verts = np.frombuffer(body[:15 * n], dtype=PLY_VERTEX)
    rec = np.frombuffer(body[15 * n:], dtype=np.uint8).reshape(m, 13)
    assert (rec[:, 0] == 3).all()
    return lines, verts, np.ascontiguousarray(rec[:, 1:]).view("<i4").reshape(m, 3)


def test_mesh_ply_container():
    from patchrefinerv2_amd import output as O
    d = _depth(37, 53, seed=37)
    img = _image(20, 31, 2)
    v = O.pointcloud_host(d, img, K)
    f = O.mesh_faces_host(d)
    rec = O.mesh_face_records(f)
    assert rec.dtype.itemsize == 13 and rec.size == f.shape[0] > 0
    data = O.mesh_ply_bytes(v.size, v.tobytes(), rec.size, rec.tobytes())
    assert data.startswith(O.mesh_ply_header(v.size, rec.size))
    cloud_head = O.ply_header(v.size).decode("ascii").split("\n")
    lines, verts, faces = _read_ply(data)
    assert lines[:-1] == cloud_head[:-2] + [f"element face {rec.size}", "property list uchar int vertex_indices"]
    assert lines[len(cloud_head) - 3] == "property uchar blue" and lines[2] == f"element vertex {v.size}"
    assert verts.tobytes() == v.tobytes() and np.array_equal(faces, f)
    # the vertex block is the body of the cloud's file
    assert data[len(O.mesh_ply_header(v.size, rec.size)):][:15 * v.size] == O.ply_bytes(v.size, v.tobytes())[len(O.ply_header(v.size)):]
    # longer buffers (the device route's bounds) are cut at 15 N and 13 M; shorter ones are errors
    assert O.mesh_ply_bytes(v.size, v.tobytes() + b"xx", rec.size, rec.tobytes() + b"yyy") == data
    with pytest.raises(ValueError):
        O.mesh_ply_bytes(v.size + 1, v.tobytes(), rec.size, rec.tobytes())
    with pytest.raises(ValueError):
        O.mesh_ply_bytes(v.size, v.tobytes(), rec.size + 1, rec.tobytes())
    # an empty mesh is a valid file
    lines, verts, faces = _read_ply(O.mesh_ply_bytes(0, b"", 0, b""))
    assert verts.size == 0 and faces.shape == (0, 3)


def _arg_count(hdr, name):
    proto = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
    return len([a for a in proto.split(",") if a.strip()])


def test_entry_points_declared_bound_exported_and_op_registered():
    from patchrefinerv2_amd import lib as L, ops, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20 and "Mesh export" in hdr
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.SIGNATURES and hasattr(raw, name), name
        assert _arg_count(hdr, name) == len(L.SIGNATURES[name][1]), name
    assert L.load().prv2_abi_version() == 20
    t = torch_ops.load()
    assert "mesh_pack" in torch_ops.OPS and hasattr(ops, "mesh_pack")
    t.mesh_pack.default._schema
    with pytest.raises((NotImplementedError, RuntimeError)):  # no CPU implementation to fall into
        t.mesh_pack(torch.zeros(1, 4, 4), torch.zeros(1, 3, 4, 4), [1.0, 1.0, 2.0, 2.0], 0.0, 1.0, 0.05, 1,
                    torch.zeros(1, 240, dtype=torch.uint8), torch.zeros(1, 234, dtype=torch.uint8))


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    err = lambda: lib.prv2_last_error().decode()  # noqa: E731
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)  # never dereferenced: every call fails its argument check before a launch
    inf = float("inf")
    assert lib.prv2_mesh_bound(30, 40, 3) == 26 * 9 * 13 and lib.prv2_mesh_bound(30, 40, 1) == 26 * 29 * 39
    assert lib.prv2_mesh_bound(1, 40, 1) == 0 and lib.prv2_mesh_bound(30, 40, 40) == 0 and lib.prv2_mesh_bound(30, 40, 0) == -1
    assert lib.prv2_mesh_bound(0, 40, 1) == -1
    assert lib.prv2_mesh_bound(20000, 26000, 1) == 26 * 19999 * 25999 > 2 ** 31  # (an int64)
    ws = lib.prv2_mesh_workspace_bytes(2, 100, 100, 1)
    assert ws == 2 * 4 * (100 * 100 + 5)  # the index map and the runs of 2048 cells: ceil(99 * 99 / 2048) = 5
    assert lib.prv2_mesh_workspace_bytes(2, 100, 100, 3) == 2 * 4 * (34 * 34 + 1)
    assert lib.prv2_mesh_workspace_bytes(1, 1, 7, 1) == 4 * 7  # no cell, no run
    assert lib.prv2_mesh_workspace_bytes(0, 4, 4, 1) == -1 and lib.prv2_mesh_workspace_bytes(1, 4, 4, 0) == -1
    cws = lib.prv2_pointcloud_workspace_bytes(2, 100, 100)

    def index(depth=p, n=2, h=100, stride=1, cwsp=p, cwsb=cws, wsp=p, wsb=ws):
        return lib.prv2_mesh_index(depth, n, h, 100, 0.0, inf, 0.05, stride, cwsp, cwsb, wsp, wsb, None)
    assert index(depth=None) != 0 and "null" in err()
    assert index(n=0) != 0 and "frame count" in err()
    assert index(h=0) != 0 and "shape" in err()
    assert index(stride=0) != 0 and "stride" in err()
    assert index(wsp=None) != 0 and "workspace" in err()
    assert index(wsp=odd) != 0 and "aligned" in err()
    assert index(wsb=ws - 1) != 0 and "workspace" in err()
    assert index(cwsp=None) != 0 and "cloud" in err()
    assert index(cwsp=odd) != 0 and "cloud" in err()
    assert index(cwsb=cws - 1) != 0 and "cloud workspace" in err()

    def count(depth=p, n=2, stride=1, counts=p, wsp=p, wsb=ws):
        return lib.prv2_mesh_count(depth, n, 100, 100, 0.05, stride, counts, wsp, wsb, None)
    assert count(depth=None) != 0 and "null" in err()
    assert count(counts=None) != 0 and "null" in err()
    assert count(n=70000) != 0 and "frame count" in err()
    assert count(stride=0) != 0 and "stride" in err()
    assert count(wsp=None) != 0 and "workspace" in err()
    assert count(wsp=odd) != 0 and "aligned" in err()
    assert count(wsb=ws - 1) != 0 and "workspace" in err()

    bound = lib.prv2_mesh_bound(100, 100, 1)

    def pack(depth=p, faces=p, fstride=bound, stride=1, wsp=p, wsb=ws):
        return lib.prv2_mesh_pack(depth, 2, 100, 100, 0.05, stride, wsp, wsb, faces, fstride, None)
    assert pack(depth=None) != 0 and "null" in err()
    assert pack(faces=None) != 0 and "null" in err()
    assert pack(fstride=bound - 1) != 0 and "stride" in err()
    assert pack(stride=0) != 0 and "stride" in err()
    assert pack(wsb=ws - 1) != 0 and "workspace" in err()
    with pytest.raises(RuntimeError):
        L.check(pack(faces=None), "mesh_pack")


def test_wrapper_validates_before_touching_the_gpu():
    from patchrefinerv2_amd import ops
    with pytest.raises(ValueError, match="GPU"):  # a host depth map
        ops.mesh_pack(torch.zeros(1, 4, 4), torch.zeros(1, 3, 4, 4), [5.0, 5.0, 2.0, 2.0])


def test_cli_save_mesh_needs_save():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "no_such_config.py", "--save-mesh"], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and "need --save" in r.stderr, r.stderr[-2000:]


def test_tester_host_route_writes_the_specification(tmp_path):
    """Tester._emit without a stage: <name>_mesh.ply comes from the host specification at the result's grid; the other files do
    not depend on the flag, and without it the set of files is the one from before"""
    from patchrefinerv2_amd import output as O
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    d = torch.from_numpy(_depth(24, 40, seed=3, holes=False)[None, None])
    img = torch.from_numpy(_image(24, 40, 1))
    item = dict(img_file_basename="f", image_hr=img[None])

    def run(work, **flags):
        info = RunnerInfo(save=True, work_dir=str(tmp_path / work), fov=70.0, ply_stride=2, ply_edge_thr=0.3, **flags)
        t = Tester(None, info, None, None)
        t._emit([], item, d, None, (24, 40))
        return {n: (tmp_path / work / n).read_bytes() for n in sorted(os.listdir(tmp_path / work))}

    t = Tester(None, RunnerInfo(save=False, work_dir=str(tmp_path), save_mesh=True), None, None)
    assert t._geometry(d, (24, 40)) is None  # nothing without save
    plain = run("plain")
    assert set(plain) == {"f.png", "f_uint16.png", "f_edge.png"}
    assert run("off", save_mesh=False, save_ply=False, save_normals=False) == plain
    cloud = run("cloud", save_ply=True, save_normals=True)
    assert set(cloud) == set(plain) | {"f.ply", "f_normal.png"}
    both = run("both", save_ply=True, save_normals=True, save_mesh=True)
    assert set(both) == set(cloud) | {"f_mesh.ply"} and {n: v for n, v in both.items() if n != "f_mesh.ply"} == cloud
    mesh = run("mesh", save_mesh=True)
    assert set(mesh) == set(plain) | {"f_mesh.ply"} and mesh["f_mesh.ply"] == both["f_mesh.ply"]
    k = O.camera_intrinsics((24, 40), (24, 40), fov=70.0)
    v = O.pointcloud_host(d[0, 0].numpy(), img.numpy(), k, edge_thr=0.3, stride=2)
    rec = O.mesh_face_records(O.mesh_faces_host(d[0, 0].numpy(), edge_thr=0.3, stride=2))
    assert rec.size > 0 and mesh["f_mesh.ply"] == O.mesh_ply_bytes(v.size, v.tobytes(), rec.size, rec.tobytes())
    _, verts, faces = _read_ply(mesh["f_mesh.ply"])
    assert verts.tobytes() == cloud["f.ply"][len(O.ply_header(v.size)):] and faces.shape == (rec.size, 3)
