"""CPU: the host half of the adaptive mesh export (patchrefinerv2_amd/output.py: mesh_adaptive_host).  The structural properties of the
specification (no T-junction, no repeated directed edge, one winding, a vertex list that is exactly the pixels used), a plain recursive
restatement it must equal, hand-checkable cases, the PLY file, the C entry points (declared, bound, exported, rejecting bad arguments
without a GPU), the CLI's argument errors and the tester's host route."""
import ctypes
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("prv2_mesh_adaptive_workspace_bytes", "prv2_mesh_adaptive_vertex_bound", "prv2_mesh_adaptive_face_bound", "prv2_mesh_adaptive_count",
           "prv2_mesh_adaptive_pack")
F32 = np.float32
K = np.array([50.0, 55.0, 19.5, 14.25], dtype=F32)  # fx, fy, cx, cy
INF = float("inf")


def _image(h, w, seed=0):
    return np.random.RandomState(seed).rand(3, h, w).astype(F32)


def _scene(h, w, seed=0, noise=1e-3, holes=True, step=True):
    """a plane that is affine in inverse depth, a fronto-parallel inset at depth 1.5 (a depth step all round it), a NaN hole, single
    pixels of every invalid kind, and relative noise"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 1.0 / (0.5 + 0.001 * x + 0.002 * y)
    if step and h > 8 and w > 8:
        d[2 * h // 7:4 * h // 7, 3 * w // 10:6 * w // 10] = 1.5
    d = d * (1.0 + noise * (2.0 * rs.rand(h, w) - 1.0))
    d = d.astype(F32)
    if holes and h * w > 40:
        d[5 * h // 7:5 * h // 7 + max(1, h // 14), 7 * w // 10:8 * w // 10] = np.nan
        idx = rs.choice(h * w, size=5, replace=False)
        d.reshape(-1)[idx] = np.array([np.nan, np.inf, -np.inf, 0.0, -1.5], dtype=F32)
    return d


def _reference(depth, depth_range=(0.0, INF), edge_thr=0.05, tolerance=0.01, block=32):
    """the rule in plain Python: loops over blocks, recursion over triangles, ``required`` by its recursive definition -> (used pixels
    ascending, faces [M, 3] into them)"""
    from patchrefinerv2_amd.output import keep_mask_host
    d = np.asarray(depth, dtype=F32)
    h, w = d.shape
    if h < 2 or w < 2:
        return np.zeros((0,), np.int64), np.zeros((0, 3), "<i4")
    B, L = int(block), int(block).bit_length() - 1
    Hp, Wp = B * -(-(h - 1) // B) + 1, B * -(-(w - 1) // B) + 1
    keep = keep_mask_host(d, depth_range, edge_thr, 1)
    thr, T = F32(edge_thr), F32(tolerance)

    def kept(p):
        return 0 <= p[0] < h and 0 <= p[1] < w and bool(keep[p])

    def joined(p, q):
        with np.errstate(all="ignore"):
            return not thr > 0 or not (abs(F32(d[p] - d[q])) > F32(thr * min(d[p], d[q])))

    def smooth(p):
        if not kept(p):
            return False
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                q = (p[0] + dy, p[1] + dx)
                if (dy or dx) and 0 <= q[0] < h and 0 <= q[1] < w and not (keep[q] and joined(p, q)):
                    return False
        return True

    def tz(v):
        return L if v == 0 else min(L, (v & -v).bit_length() - 1)

    def parts(p):
        """-> (hypotenuse ends, existing apexes, existing child vertices) of a vertex that is not a block corner"""
        y, x = p
        hh = 1 << min(tz(y), tz(x))
        if (y // hh) % 2 and (x // hh) % 2:
            if 2 * hh == B:
                main = True
            else:
                pcy, pcx = (y // (4 * hh)) * 4 * hh + 2 * hh, (x // (4 * hh)) * 4 * hh + 2 * hh
                main = (y - pcy > 0) == (x - pcx > 0)
            diag, anti = [(y - hh, x - hh), (y + hh, x + hh)], [(y - hh, x + hh), (y + hh, x - hh)]
            ends, apex = (diag, anti) if main else (anti, diag)
            kids = [(y - hh, x), (y + hh, x), (y, x - hh), (y, x + hh)]
        else:
            along_x = bool((x // hh) % 2)
            ends = [(y, x - hh), (y, x + hh)] if along_x else [(y - hh, x), (y + hh, x)]
            apex = [(y - hh, x), (y + hh, x)] if along_x else [(y, x - hh), (y, x + hh)]
            q = hh // 2
            kids = [(y - q, x - q), (y - q, x + q), (y + q, x - q), (y + q, x + q)] if q else []
        inside = lambda v: 0 <= v[0] < Hp and 0 <= v[1] < Wp  # noqa: E731
        assert all(inside(e) for e in ends)
        return ends, [a for a in apex if inside(a)], [k for k in kids if inside(k)]

    @functools.lru_cache(maxsize=None)
    def required(p):
        ends, apex, kids = parts(p)
        if not smooth(p) or not all(kept(v) for v in ends + apex) or any(required(k) for k in kids):
            return True
        with np.errstate(all="ignore"):
            za, zb, zm = d[ends[0]], d[ends[1]], d[p]
            s = F32(za + zb)
            pp, qq = F32(zm * s), F32(F32(za * zb) * F32(2))
            return bool(abs(F32(pp - qq)) > F32(T * pp))

    out = []

    def walk(a, b, c, k):
        if k == 2 * L:
            if kept(a) and kept(b) and kept(c) and joined(a, b) and joined(b, c) and joined(a, c):
                out.append((a, b, c))
            return
        m = ((a[0] + b[0]) // 2, (a[1] + b[1]) // 2)
        if not required(m):
            out.append((a, b, c))
            return
        walk(c, a, m, k + 1)
        walk(b, c, m, k + 1)

    for y0 in range(0, Hp - 1, B):
        for x0 in range(0, Wp - 1, B):
            A, Bp, C, D = (y0, x0), (y0, x0 + B), (y0 + B, x0), (y0 + B, x0 + B)
            walk(D, A, C, 0)
            walk(A, D, Bp, 0)
    pix = np.array([[p[0] * w + p[1] for p in t] for t in out], dtype=np.int64).reshape(-1, 3)
    used = np.unique(pix)
    return used, np.searchsorted(used, pix).astype("<i4")


def _check_structure(depth, used, faces, depth_range=(0.0, INF), edge_thr=0.05):
    """what every adaptive mesh has: a vertex list that is exactly the kept pixels its faces use, in pixel order; no used vertex
    strictly inside an edge of a face (no T-junction); no directed edge twice; every face wound like the faces of mesh_faces_host"""
    from patchrefinerv2_amd.output import keep_mask_host
    h, w = depth.shape
    assert used.dtype == np.int64 and used.ndim == 1 and faces.dtype == np.dtype("<i4") and faces.ndim == 2 and faces.shape[1] == 3
    assert (np.diff(used) > 0).all()
    if not faces.size:
        assert not used.size
        return
    assert faces.min() >= 0 and faces.max() < used.size
    assert np.array_equal(np.unique(faces), np.arange(used.size))  # every listed vertex is referenced
    assert used.min() >= 0 and used.max() < h * w and keep_mask_host(depth, depth_range, edge_thr, 1).reshape(-1)[used].all()
    py, px = np.divmod(used[faces], w)  # [M, 3]
    cross = (px[:, 1] - px[:, 0]) * (py[:, 2] - py[:, 0]) - (py[:, 1] - py[:, 0]) * (px[:, 2] - px[:, 0])
    assert (cross < 0).all()  # (TL, BL, BR) of mesh_faces_host: 0 * 1 - 1 * 1
    is_used = set(used.tolist())
    directed = set()
    for f in range(faces.shape[0]):
        for i, j in ((0, 1), (1, 2), (2, 0)):
            p, q = (int(py[f, i]), int(px[f, i])), (int(py[f, j]), int(px[f, j]))
            assert (p, q) not in directed
            directed.add((p, q))
            dy, dx = q[0] - p[0], q[1] - p[1]
            n = max(abs(dy), abs(dx))
            assert n > 0 and abs(dy) in (0, n) and abs(dx) in (0, n)  # along an axis or a diagonal
            for t in range(1, n):
                assert (p[0] + t * dy // n) * w + p[1] + t * dx // n not in is_used, (p, q, t)


SHAPES = [((70, 100), 32), ((66, 100), 16), ((67, 131), 64), ((9, 13), 4), ((33, 33), 32), ((2, 2), 4), ((1, 5), 4), ((2, 3), 4), ((5, 5), 4)]


@pytest.mark.parametrize("shape,block", SHAPES)
@pytest.mark.parametrize("tolerance", [0.0, 0.01, 1e9])
def test_structure_and_the_recursive_restatement(shape, block, tolerance):
    from patchrefinerv2_amd import output as O
    d = _scene(*shape, seed=shape[0], noise=0.004)
    used, faces = O.mesh_adaptive_host(d, tolerance=tolerance, block=block)
    _check_structure(d, used, faces)
    want_used, want_faces = _reference(d, tolerance=tolerance, block=block)
    assert np.array_equal(used, want_used) and np.array_equal(faces, want_faces)
    if min(shape) >= 2:
        assert faces.shape[0] > 0


@pytest.mark.parametrize("seed", range(6))
def test_structure_over_seeds(seed):
    """noise from 0 to 1 %, blocks from 2 to 16, other depth ranges and thresholds"""
    from patchrefinerv2_amd import output as O
    rs = np.random.RandomState(seed)
    h, w = int(rs.randint(20, 60)), int(rs.randint(20, 60))
    d = _scene(h, w, seed=seed, noise=[0.0, 0.001, 0.002, 0.005, 0.01, 0.003][seed])
    kw = dict(depth_range=[(0.0, INF), (1.2, 1.9)][seed % 2], edge_thr=[0.05, 0.0, 0.02][seed % 3])
    tol, block = [0.0, 0.002, 0.01, 0.05, 1e9, 0.005][seed], [2, 4, 8, 16, 8, 4][seed]
    used, faces = O.mesh_adaptive_host(d, tolerance=tol, block=block, **kw)
    assert faces.shape[0] > 0
    _check_structure(d, used, faces, **kw)
    want_used, want_faces = _reference(d, tolerance=tol, block=block, **kw)
    assert np.array_equal(used, want_used) and np.array_equal(faces, want_faces)


@pytest.mark.parametrize("k,j,block", [(1, 1, 4), (2, 3, 8), (1, 2, 32), (3, 1, 2)])
def test_a_plane_gives_two_faces_a_block(k, j, block):
    from patchrefinerv2_amd import output as O
    d = _scene(k * block + 1, j * block + 1, noise=0.0, holes=False, step=False)
    used, faces = O.mesh_adaptive_host(d, tolerance=1e-4, block=block)
    assert faces.shape[0] == 2 * k * j and used.size == (k + 1) * (j + 1)
    w = j * block + 1
    assert sorted(used.tolist()) == sorted(y * block * w + x * block for y in range(k + 1) for x in range(j + 1))
    if (k, j) == (1, 1):  # (D, A, C) then (A, D, B'): A, B', C, D are the vertices 0, 1, 2, 3
        assert faces.tolist() == [[3, 0, 2], [0, 3, 1]]
    _check_structure(d, used, faces)


def _faces_per_block(used, faces, w, block, shape):
    py, px = np.divmod(used[faces], w)
    blk = (py.min(axis=1) // block) * shape[1] + px.min(axis=1) // block
    return np.bincount(blk, minlength=shape[0] * shape[1]).reshape(shape)


def test_a_huge_tolerance_refines_only_around_defects():
    """T = 1e9 switches the geometric test off: a noisy map without defects has two faces a block; one invalid pixel inside block
    (0, 0) refines that block and, through the shared border, at most its three neighbours"""
    from patchrefinerv2_amd import output as O
    B = 32
    d = _scene(3 * B + 1, 3 * B + 1, seed=4, noise=0.01, holes=False, step=False)
    used, faces = O.mesh_adaptive_host(d, tolerance=1e9, block=B)
    assert faces.shape[0] == 18 and used.size == 16
    d[10, 13] = np.nan
    used, faces = O.mesh_adaptive_host(d, tolerance=1e9, block=B)
    _check_structure(d, used, faces)
    per = _faces_per_block(used, faces, d.shape[1], B, (3, 3))
    assert per[0, 0] > 2 and (per[2, :] == 2).all() and (per[:, 2] == 2).all()
    # Pixel-sized triangles only next to the hole.  Their apex is a vertex at hh = 1 that is required: it is not smooth (the hole is
    # one of its 8 neighbours) or, a centre, has such a child vertex one pixel away; the other two corners are its neighbours.  So
    # no corner is more than 3 pixels from the hole.
    py, px = np.divmod(used[faces], d.shape[1])
    small = ((py.max(axis=1) - py.min(axis=1)) == 1) & ((px.max(axis=1) - px.min(axis=1)) == 1)
    assert small.any() and (np.abs(py[small] - 10).max() <= 3) and (np.abs(px[small] - 13).max() <= 3)


def test_zero_tolerance_covers_the_cells_of_the_stride_one_mesh():
    """T = 0 on a noisy map: every triangle is a finest one.  A cell whose four corners are kept and pairwise joined has its two
    faces in both meshes; the others (beside defects) differ at most by the diagonal, which here is the hierarchy's"""
    from patchrefinerv2_amd import output as O
    h, w, B = 70, 100, 32
    d = _scene(h, w, seed=7, noise=0.002)
    used, faces = O.mesh_adaptive_host(d, tolerance=0.0, block=B)
    _check_structure(d, used, faces)
    py, px = np.divmod(used[faces], w)
    assert ((py.max(axis=1) - py.min(axis=1)) == 1).all() and ((px.max(axis=1) - px.min(axis=1)) == 1).all()
    got = np.bincount(py.min(axis=1) * (w - 1) + px.min(axis=1), minlength=(h - 1) * (w - 1)).reshape(h - 1, w - 1)
    keep = O.keep_mask_host(d)
    thr = F32(0.05)
    c = [(slice(None, -1), slice(None, -1)), (slice(None, -1), slice(1, None)), (slice(1, None), slice(None, -1)), (slice(1, None), slice(1, None))]
    clean = keep[c[0]] & keep[c[1]] & keep[c[2]] & keep[c[3]]
    with np.errstate(all="ignore"):
        for a in range(4):
            for b in range(a + 1, 4):
                clean &= ~(np.abs(d[c[a]] - d[c[b]]) > thr * np.minimum(d[c[a]], d[c[b]]))
    assert (got[clean] == 2).all() and clean.sum() > 0.9 * clean.size
    full = O.mesh_faces_host(d).shape[0]
    assert 2 * clean.sum() <= faces.shape[0] <= 2 * clean.sum() + 2 * (~clean).sum() and abs(full - faces.shape[0]) <= 2 * (~clean).sum()


def test_no_edge_threshold_invalid_frames_and_thin_frames():
    from patchrefinerv2_amd import output as O
    B = 8
    d = _scene(2 * B + 1, 3 * B + 1, seed=2, noise=0.01, holes=False, step=True)
    used, faces = O.mesh_adaptive_host(d, edge_thr=0.0, tolerance=1e9, block=B)  # every pixel kept and joined: the step does not split
    assert faces.shape[0] == 12 and used.size == 12
    used, faces = O.mesh_adaptive_host(d, edge_thr=-1.0, tolerance=0.0, block=B)
    assert faces.shape[0] == 2 * 2 * B * 3 * B and used.size == d.size
    assert np.array_equal(faces, _reference(d, edge_thr=-1.0, tolerance=0.0, block=B)[1])
    used, faces = O.mesh_adaptive_host(d, tolerance=1e9, block=B)  # with the threshold the step's flying pixels are holes
    assert faces.shape[0] > 12
    for empty in (np.full((20, 30), np.nan, dtype=F32), np.full((1, 9), 2.0, dtype=F32), np.full((9, 1), 2.0, dtype=F32), np.full((1, 1), 2.0, dtype=F32)):
        used, faces = O.mesh_adaptive_host(empty, tolerance=0.01, block=4)
        assert used.shape == (0,) and used.dtype == np.int64 and faces.shape == (0, 3) and faces.dtype == np.dtype("<i4")
    for bad in (dict(tolerance=-0.1), dict(tolerance=float("nan")), dict(tolerance=INF), dict(block=1), dict(block=24), dict(block=128), dict(block=0)):
        with pytest.raises(ValueError):
            O.mesh_adaptive_host(d, **{**dict(tolerance=0.01, block=8), **bad})


def test_the_mesh_is_less_than_half_the_full_one():
    """the scene and the tolerance of the README row's small sibling: a plane, an inset, a hole, 0.1 % noise at T = 0.01"""
    from patchrefinerv2_amd import output as O
    d = _scene(70, 100, seed=0, noise=0.001)
    used, faces = O.mesh_adaptive_host(d, tolerance=0.01, block=32)
    full, cloud = O.mesh_faces_host(d).shape[0], int(O.keep_mask_host(d).sum())
    assert full > 12000 and 0 < faces.shape[0] < full // 2 and 0 < used.size < cloud // 2


def test_a_large_frame_takes_seconds():
    import time
    from patchrefinerv2_amd import output as O
    d = np.tile(_scene(270, 480, seed=1), (8, 8))
    t0 = time.time()
    used, faces = O.mesh_adaptive_host(d, tolerance=0.01, block=32)
    assert d.shape == (2160, 3840) and faces.shape[0] > 0 and time.time() - t0 < 60.0


def _read_ply(data):
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
    return verts, np.ascontiguousarray(rec[:, 1:]).view("<i4").reshape(m, 3)


def test_files(tmp_path):
    """<name>_mesh.ply with the tolerance parses back to the specification's vertices and faces; the cloud beside it, and every file
    written without the new arguments, is what it was"""
    from patchrefinerv2_amd import output as O
    d, img = _scene(37, 53, seed=3), _image(20, 31, 2)
    geo = dict(depth_range=(0.0, INF), edge_thr=0.05)
    cloud = O.pointcloud_host(d, img, K, **geo)
    grid = O.mesh_face_records(O.mesh_faces_host(d, **geo))
    for work in ("old", "new", "alias"):
        (tmp_path / work).mkdir()
    O.write_geometry_host(str(tmp_path / "old" / "f"), d, img, K, ply=True, normals=True, mesh=True, **geo)
    O.write_geometry_host(str(tmp_path / "new" / "f"), d, img, K, ply=True, normals=True, mesh=True, mesh_tolerance=0.01, mesh_block=8, **geo)
    O.save_geometry_host(str(tmp_path / "alias" / "f"), d, img, K, ply=False, normals=False, mesh=True, mesh_tolerance=0.01, mesh_block=8, **geo)
    read = lambda work: {n: (tmp_path / work / n).read_bytes() for n in sorted(os.listdir(tmp_path / work))}  # noqa: E731
    old, new, alias = read("old"), read("new"), read("alias")
    assert set(old) == set(new) == {"f.ply", "f_normal.png", "f_mesh.ply"} and set(alias) == {"f_mesh.ply"}
    assert old["f.ply"] == O.ply_bytes(cloud.size, cloud.tobytes()) == new["f.ply"] and old["f_normal.png"] == new["f_normal.png"]
    assert old["f_mesh.ply"] == O.mesh_ply_bytes(cloud.size, cloud.tobytes(), grid.size, grid.tobytes())
    assert alias["f_mesh.ply"] == new["f_mesh.ply"] != old["f_mesh.ply"]
    used, faces = O.mesh_adaptive_host(d, tolerance=0.01, block=8, **geo)
    verts, tri = _read_ply(new["f_mesh.ply"])
    assert np.array_equal(tri, faces) and 0 < verts.size == used.size < cloud.size
    assert new["f_mesh.ply"].startswith(O.mesh_ply_header(used.size, faces.shape[0]))
    # a vertex is the cloud's record of its pixel
    rank = np.cumsum(O.keep_mask_host(d, **geo).reshape(-1)) - 1
    assert verts.tobytes() == cloud[rank[used]].tobytes() == O.mesh_adaptive_vertices(d, img, K, used, **geo).tobytes()
    with pytest.raises(ValueError, match="stride"):
        O.write_geometry_host(str(tmp_path / "new" / "g"), d, img, K, mesh=True, mesh_tolerance=0.01, stride=2, **geo)


def _arg_count(hdr, name):
    proto = re.search(rf"\b{name}\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
    return len([a for a in proto.split(",") if a.strip()])


def test_entry_points_declared_bound_exported_and_op_registered():
    from patchrefinerv2_amd import lib as L, ops, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20 and "Adaptive mesh export" in hdr
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr) and name in L.SIGNATURES and hasattr(raw, name), name
        assert _arg_count(hdr, name) == len(L.SIGNATURES[name][1]), name
    assert L.load().prv2_abi_version() == 20
    t = torch_ops.load()
    assert "mesh_adaptive_pack" in torch_ops.OPS and hasattr(ops, "mesh_adaptive_pack")
    t.mesh_adaptive_pack.default._schema
    with pytest.raises((NotImplementedError, RuntimeError)):  # no CPU implementation to fall into
        t.mesh_adaptive_pack(torch.zeros(1, 4, 4), torch.zeros(1, 3, 4, 4), [1.0, 1.0, 2.0, 2.0], 0.0, 1.0, 0.05, 0.01, 4,
                             torch.zeros(1, 240, dtype=torch.uint8), torch.zeros(1, 234, dtype=torch.uint8))


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    err = lambda: lib.prv2_last_error().decode()  # noqa: E731
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)  # never dereferenced: every call fails its argument check before a launch
    nan = float("nan")
    assert lib.prv2_mesh_adaptive_vertex_bound(30, 40) == 15 * 30 * 40 and lib.prv2_mesh_adaptive_face_bound(30, 40) == 26 * 29 * 39
    assert lib.prv2_mesh_adaptive_face_bound(1, 40) == 0 and lib.prv2_mesh_adaptive_face_bound(0, 40) == -1
    assert lib.prv2_mesh_adaptive_vertex_bound(30, 0) == -1
    assert lib.prv2_mesh_adaptive_face_bound(20000, 26000) == 26 * 19999 * 25999 > 2 ** 31  # (an int64)
    # 70 x 100 in blocks of 32: 97 x 129 vertices, 2 * 96 * 128 slots = 12 runs, 12513 vertices = 7 runs
    ws = lib.prv2_mesh_adaptive_workspace_bytes(2, 70, 100, 32)
    assert ws == 2 * (6 * 97 * 129 + 4 * 12 + 4 * 7)
    assert lib.prv2_mesh_adaptive_workspace_bytes(1, 33, 33, 32) == 6 * 33 * 33 + 4 * 1 + 4 * 1 + 2  # (rounded up to 4)
    assert lib.prv2_mesh_adaptive_workspace_bytes(1, 1, 7, 4) == 4  # no cell
    for bad in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 4, 3), (1, 4, 4, 1), (1, 4, 4, 128), (1, 4, 4, 0), (70000, 4, 4, 4), (1, 2, 8388608, 64)):
        assert lib.prv2_mesh_adaptive_workspace_bytes(*bad) == -1, bad

    def count(depth=p, n=2, h=70, tol=0.01, block=32, nv=p, nf=p, wsp=p, wsb=ws, lo=0.0, thr=0.05):
        return lib.prv2_mesh_adaptive_count(depth, n, h, 100, lo, INF, thr, tol, block, nv, nf, wsp, wsb, None)
    assert count(depth=None) != 0 and "null" in err()
    assert count(nv=None) != 0 and "null" in err()
    assert count(nf=None) != 0 and "null" in err()
    assert count(n=0) != 0 and "frame count" in err()
    assert count(h=0) != 0 and "shape" in err()
    assert count(lo=nan) != 0 and "NaN" in err()
    assert count(thr=nan) != 0 and "NaN" in err()
    for tol in (nan, -0.5, INF, -INF):
        assert count(tol=tol) != 0 and "tolerance" in err(), tol
    for block in (0, 1, 3, 48, 128, -32):
        assert count(block=block) != 0 and "block" in err(), block
    assert count(wsp=None) != 0 and "workspace" in err()
    assert count(wsp=odd) != 0 and "aligned" in err()
    assert count(wsb=ws - 1) != 0 and "workspace" in err()
    assert count(block=64) != 0 and "workspace" in err()  # (more padding than the workspace was sized for)

    vb, fb = lib.prv2_mesh_adaptive_vertex_bound(70, 100), lib.prv2_mesh_adaptive_face_bound(70, 100)

    def pack(depth=p, image=p, ih=20, fx=50.0, tol=0.01, block=32, wsp=p, wsb=ws, verts=p, vs=vb, faces=p, fs=fb):
        return lib.prv2_mesh_adaptive_pack(depth, image, 2, 70, 100, ih, 30, fx, 50.0, 1.0, 1.0, 0.0, INF, 0.05, tol, block, wsp, wsb, verts, vs,
                                           faces, fs, None)
    assert pack(depth=None) != 0 and "null" in err()
    assert pack(image=None) != 0 and "null" in err()
    assert pack(verts=None) != 0 and "null" in err()
    assert pack(faces=None) != 0 and "null" in err()
    assert pack(ih=0) != 0 and "image" in err()
    assert pack(fx=0.0) != 0 and "focal" in err()
    assert pack(tol=nan) != 0 and "tolerance" in err()
    assert pack(tol=-1.0) != 0 and "tolerance" in err()
    assert pack(block=12) != 0 and "block" in err()
    assert pack(wsp=None) != 0 and "workspace" in err()
    assert pack(wsb=ws - 1) != 0 and "workspace" in err()
    assert pack(vs=vb - 1) != 0 and "vertex buffer" in err()
    assert pack(fs=fb - 1) != 0 and "face buffer" in err()
    with pytest.raises(RuntimeError):
        L.check(pack(faces=None), "mesh_adaptive_pack")


def test_wrapper_validates_before_touching_the_gpu():
    from patchrefinerv2_amd import ops
    d, img, k = torch.zeros(1, 4, 4), torch.zeros(1, 3, 4, 4), [5.0, 5.0, 2.0, 2.0]
    with pytest.raises(ValueError, match="GPU"):  # a host depth map
        ops.mesh_adaptive_pack(d, img, k)
    for bad in (dict(tolerance=-1.0), dict(tolerance=float("nan")), dict(tolerance=INF), dict(block=3), dict(block=128), dict(block=1)):
        with pytest.raises(ValueError, match="tolerance|block"):
            ops.mesh_adaptive_pack(d, img, k, **bad)


@pytest.mark.parametrize("flags,message", [
    (["--mesh-tolerance", "0.01"], "--mesh-tolerance needs --save-mesh"),
    (["--save", "--save-mesh", "--mesh-tolerance", "0.01", "--ply-stride", "2"], "has no stride"),
    (["--save", "--save-mesh", "--mesh-tolerance", "-0.01"], "finite and at least 0"),
    (["--save", "--save-mesh", "--mesh-tolerance", "nan"], "finite and at least 0"),
    (["--save", "--save-mesh", "--mesh-tolerance", "0.01", "--mesh-block", "24"], "power of two"),
])
def test_cli_argument_errors(flags, message):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "no_such_config.py"] + flags, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and message in r.stderr, r.stderr[-2000:]


def test_tester_host_route_writes_the_specification(tmp_path):
    """Tester._emit without a stage: with ``mesh_tolerance`` <name>_mesh.ply is the adaptive mesh at the result's grid; the other files
    do not depend on it, and without it the files are the ones from before"""
    from patchrefinerv2_amd import output as O
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    d = torch.from_numpy(_scene(24, 40, seed=3)[None, None])
    img = torch.from_numpy(_image(24, 40, 1))
    item = dict(img_file_basename="f", image_hr=img[None])

    def run(work, **flags):
        info = RunnerInfo(save=True, work_dir=str(tmp_path / work), fov=70.0, ply_edge_thr=0.3, **flags)
        t = Tester(None, info, None, None)
        t._emit([], item, d, None, (24, 40))
        return {n: (tmp_path / work / n).read_bytes() for n in sorted(os.listdir(tmp_path / work))}

    grid = run("grid", save_ply=True, save_mesh=True)
    ada = run("ada", save_ply=True, save_mesh=True, mesh_tolerance=0.02, mesh_block=8)
    assert set(ada) == set(grid) and {n: v for n, v in ada.items() if n != "f_mesh.ply"} == {n: v for n, v in grid.items() if n != "f_mesh.ply"}
    k = O.camera_intrinsics((24, 40), (24, 40), fov=70.0)
    used, faces = O.mesh_adaptive_host(d[0, 0].numpy(), edge_thr=0.3, tolerance=0.02, block=8)
    v, rec = O.mesh_adaptive_vertices(d[0, 0].numpy(), img.numpy(), k, used, edge_thr=0.3), O.mesh_face_records(faces)
    assert rec.size > 0 and ada["f_mesh.ply"] == O.mesh_ply_bytes(v.size, v.tobytes(), rec.size, rec.tobytes()) != grid["f_mesh.ply"]
    assert run("default", save_mesh=True, mesh_tolerance=0.02)["f_mesh.ply"] == run("b32", save_mesh=True, mesh_tolerance=0.02, mesh_block=32)["f_mesh.ply"]
    for bad in (dict(save_mesh=False, save_ply=True), dict(save_mesh=True, ply_stride=2), dict(save_mesh=True, mesh_block=5),
                dict(save_mesh=True, mesh_tolerance=-1.0)):
        t = Tester(None, RunnerInfo(save=True, work_dir=str(tmp_path), **{**dict(mesh_tolerance=0.02), **bad}), None, None)
        with pytest.raises(ValueError):
            t._geometry(d, (24, 40))
