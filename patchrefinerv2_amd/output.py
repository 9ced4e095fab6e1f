"""GPU output stage of the tester (opt-in: ``runner_info.device_output`` / ``tools/test.py --device-output``).

The files ``Tester.run(save=True)`` and ``Tester.generate_pl(save=True)`` write are PNGs of per-pixel functions of maps that
are already on the device.  This module produces the deflate-ready scanlines of every file there (csrc/output.hip through
ops.py), copies only those packed bytes into pinned host memory and hands them to a bounded pool of writer threads
(``zlib.compress`` releases the GIL), while the next frame computes.  The host route's ``write_png16`` / ``write_png8`` below go
through the same container (``png_bytes``): equal pixels give byte-identical files.

``device_deflate`` (``runner_info.device_deflate`` / ``tools/test.py --device-deflate``, on top of the device route) also produces
the zlib stream of every file on the GPU (csrc/deflate.hip through ``ops.deflate_rows``): only compressed bytes are copied to the
host and the writer threads compute the chunk CRC and write.  Such files hold the same pixels as the device route's but NOT the
same bytes: the IDAT payload is the device encoder's stream, not zlib level 6's (and usually larger).

percentile_from_sorted   np.percentile(method='linear') of a float32 array from two neighbouring order statistics (host)
colormap_lut / lut_index matplotlib's byte table and index rule (host restatement: the spec of prv2_colorize_rows)
percentile_device        np.percentile(value[mask], q) of a device map (exact order statistics + the host interpolation)
colorize_device          metrics.colorize of a device map -> device uint8 [H, W, 3] view + its scanline buffer
png_bytes_from_stream    the PNG container around a given IDAT payload
write_png16 / write_png8 a host array as a PNG file (the host route's dependency-free encoder)
camera_intrinsics        fx, fy, cx, cy of a result map's grid from --intrinsics / --fov (host)
pointcloud_host / normal_map_host / ply_bytes
                         the host specification of the geometry export (csrc/pointcloud.hip equals it bit for bit) and the PLY file
mesh_faces_host / mesh_ply_bytes
                         the host specification of the mesh's faces (likewise) and the PLY file of vertices and faces
mesh_adaptive_host / mesh_adaptive_vertices
                         the host specification of the adaptive mesh (csrc/mesh_adaptive.hip equals it byte for byte): the used pixels
                         and the faces of a right-triangulated irregular network, and the vertex records of those pixels
stereo_source_host / stereo_view_host / stereo_image_host
                         the host specification of the right-eye view (csrc/stereo.hip equals it byte for byte)
bokeh_render_host / bokeh_image_host
                         the host specification of the depth-of-field view (csrc/bokeh.hip equals it bit for bit)
view_source_host / view_image_host / view_poses
                         the host specification of the views from a moved camera (csrc/view.hip equals it bit for bit) and their path
OutputStage              side stream, ring of pinned staging slots, writer pool

Geometry export (``runner_info.save_ply`` / ``save_normals``; tools/test.py --save-ply / --save-normals): <name>.ply, a binary
little-endian point cloud of the result map (float x, y, z + uchar red, green, blue per kept pixel, row-major pixel order), and
<name>_normal.png, its camera-facing surface normals.  Pinhole camera, x right, y down, z forward.  ``runner_info.save_mesh``
(--save-mesh) adds <name>_mesh.ply: the same vertices joined into camera-facing triangles along the pixel grid, two per cell of
four kept neighbours at most, none across a depth discontinuity (``mesh_faces_host``); with ``runner_info.mesh_tolerance``
(--mesh-tolerance) the file holds the adaptive mesh instead, with its own vertex list (``mesh_adaptive_host``).  ``runner_info.save_stereo`` (--save-stereo)
adds <name>_right.png (or _sbs / _anaglyph): the frame seen from a second eye ``stereo_baseline`` metres to the right
(``stereo_source_host``: a per-row forward warp with a depth test, disocclusions filled from the farther side).
``runner_info.save_bokeh`` (--save-bokeh) adds <name>_bokeh.png: the frame seen through a thin lens of ``bokeh_aperture`` metres
focused at ``bokeh_focus`` metres or at the depth under ``bokeh_focus_point`` (``bokeh_render_host``).
``runner_info.save_views`` = N (--save-views N) adds <name>_view_000.png ...: the frame seen from N poses of a closed camera path
(``view_poses``), the map's own mesh rasterised with a depth test (``view_source_host``).
"""
from __future__ import annotations

import math
import os
import struct
import threading
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

MAX_WORKERS = 16  # the cap of the writer pool (never sized from os.cpu_count(): a shared box reports every core of the machine)
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------
# host restatements (no GPU)
# ------------------------------------------------------------------------------------------------------------------
def percentile_ranks(n: int, p: float):
    """(lo, hi, g): np.percentile(a, p) of a float32 array of n values is _lerp(sort(a)[lo], sort(a)[hi], g).  numpy computes the
    virtual index in the array's dtype: q = float32(p) / float32(100), pos = float32(n - 1) * q (a float64 index does not
    reproduce it)."""
    if n < 1:
        raise ValueError("percentile of an empty set")
    q32 = F32(p) / F32(100)
    pos = F32(n - 1) * q32
    lo = int(np.floor(pos))
    g = F32(pos - F32(lo))
    lo = min(max(lo, 0), n - 1)
    return lo, min(lo + 1, n - 1), g


def lerp_f32(a, b, g):
    """numpy's _lerp on float32 scalars: a + (b - a) * g, and b - (b - a) * (1 - g) from g >= 0.5"""
    a, b, g = F32(a), F32(b), F32(g)
    with np.errstate(invalid="ignore", over="ignore"):
        d = F32(b - a)
        return F32(b - d * F32(F32(1) - g)) if g >= F32(0.5) else F32(a + d * g)


def percentile_from_sorted(s_lo, s_hi, s_last, n: int, p: float):
    """np.percentile of n float32 values given sort(a)[lo], sort(a)[hi] (``percentile_ranks``) and the largest: NaN sorts last and
    makes every percentile NaN"""
    if np.isnan(s_last):
        return F32(np.nan)
    return lerp_f32(s_lo, s_hi, percentile_ranks(n, p)[2])


def colormap_lut(cmap: str) -> np.ndarray:
    """(N + 3) x 4 uint8: what matplotlib's Colormap.__call__(bytes=True) looks its indices up in (rows N, N + 1, N + 2 =
    under, over, bad)"""
    import matplotlib
    cm = matplotlib.colormaps[cmap]
    if not cm._isinit:
        cm._init()
    return np.ascontiguousarray((cm._lut * 255).astype(np.uint8))


def lut_index(x: np.ndarray, n: int) -> np.ndarray:
    """matplotlib's index rule for float data: xa = x * N in x's dtype; xa == N -> N - 1; xa < 0 -> under (N); xa >= N -> over
    (N + 1); NaN -> bad (N + 2); else truncation"""
    xa = np.array(x, copy=True)
    with np.errstate(invalid="ignore", over="ignore"):
        xa *= n
        xa[xa == n] = n - 1
        under, over, bad = xa < 0, xa >= n, np.isnan(xa)
        idx = xa.astype(np.int64)
    idx[under], idx[over], idx[bad] = n, n + 1, n + 2
    return idx


def png_bytes_from_stream(header: bytes, zstream) -> bytes:
    """signature, IHDR, one IDAT whose payload is ``zstream`` (a zlib stream of the scanlines, taken as given), IEND"""
    def chunk(tag, data):
        crc = zlib.crc32(data, zlib.crc32(tag)) & 0xFFFFFFFF
        return struct.pack(">I", len(data)) + tag + bytes(data) + struct.pack(">I", crc)
    return PNG_SIGNATURE + chunk(b"IHDR", header) + chunk(b"IDAT", zstream) + chunk(b"IEND", b"")


def png_bytes(header: bytes, rows) -> bytes:
    """the file of these scanlines: signature, IHDR, one IDAT (zlib level 6), IEND"""
    return png_bytes_from_stream(header, zlib.compress(rows, 6))


def ihdr(w: int, h: int, bpp: int) -> bytes:
    """bpp (bytes per pixel) 1: 8-bit gray, 2: 16-bit gray, 3: 8-bit RGB, 4: 8-bit RGBA"""
    depth, ctype = {1: (8, 0), 2: (16, 0), 3: (8, 2), 4: (8, 6)}[bpp]
    return struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0)


def _write_png(path: str, samples: np.ndarray, h: int, w: int, bpp: int):
    """``samples``: the image's h * w * bpp bytes in file order -> scanlines with filter byte 0 -> ``png_bytes`` -> the file"""
    rows = np.zeros((h, 1 + bpp * w), dtype=np.uint8)
    rows[:, 1:] = samples.reshape(h, bpp * w)
    with open(path, "wb") as f:
        f.write(png_bytes(ihdr(w, h, bpp), rows.tobytes()))


def write_png16(path: str, arr_u16: np.ndarray):
    """Minimal PNG encoder: 16-bit grayscale (== PIL's Image.fromarray(uint16).save)."""
    assert arr_u16.dtype == np.uint16 and arr_u16.ndim == 2
    _write_png(path, arr_u16.astype(">u2").view(np.uint8), *arr_u16.shape, 2)


def write_png8(path: str, arr_u8: np.ndarray):
    """8-bit RGB / RGBA / gray PNG (== cv2.imwrite of the BGR-swapped array the reference builds)."""
    assert arr_u8.dtype == np.uint8 and arr_u8.ndim in (2, 3)
    ch = 1 if arr_u8.ndim == 2 else arr_u8.shape[2]
    if ch not in (1, 3, 4):
        raise ValueError(f"write_png8: {ch} channels; gray [h, w], RGB [h, w, 3] or RGBA [h, w, 4]")
    _write_png(path, arr_u8, *arr_u8.shape[:2], ch)


# ------------------------------------------------------------------------------------------------------------------
# geometry export: the host specification (numpy float32, one rounding per operation in the order written; csrc/pointcloud.hip
# equals it bit for bit) and the PLY container
# ------------------------------------------------------------------------------------------------------------------
PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])  # 15 bytes, packed


def camera_intrinsics(raw_shape, result_shape, intrinsics=None, fov=60.0) -> np.ndarray:
    """float32 [4] = fx, fy, cx, cy in pixels of the result map's grid.  ``intrinsics`` (fx, fy, cx, cy) are given in pixels of the
    ``raw_shape`` (H_raw, W_raw) grid; without them they come from ``fov``, a horizontal field of view in degrees:
    fx = fy = (W_raw / 2) / tan(fov / 2), cx = W_raw / 2, cy = H_raw / 2.  They are scaled in float64 to ``result_shape`` (H, W) --
    the m-modes return the re-ensemble shape, not the raw one: fx, cx by W / W_raw and fy, cy by H / H_raw -- and cast once."""
    hr, wr = (float(v) for v in raw_shape)
    h, w = (float(v) for v in result_shape)
    if intrinsics is None:
        if not 0.0 < float(fov) < 180.0:
            raise ValueError(f"fov {fov}: a horizontal field of view in degrees, inside (0, 180)")
        f = (wr / 2.0) / math.tan(math.radians(float(fov)) / 2.0)
        intrinsics = (f, f, wr / 2.0, hr / 2.0)
    fx, fy, cx, cy = (float(v) for v in intrinsics)
    return np.array([fx * (w / wr), fy * (h / hr), cx * (w / wr), cy * (h / hr)], dtype=np.float64).astype(F32)


def _valid_depth(d, depth_range):
    with np.errstate(invalid="ignore"):
        return np.isfinite(d) & (d > F32(depth_range[0])) & (d < F32(depth_range[1]))


def backproject_host(depth, intrinsics):
    """-> X, Y, Z float32 [h, w]: Z = D[y, x], u = (float(x) + 0.5) - cx, X = (u * Z) / fx; Y likewise with cy, fy"""
    d = np.ascontiguousarray(depth, dtype=F32)
    h, w = d.shape
    fx, fy, cx, cy = (F32(v) for v in intrinsics)
    u = (np.arange(w, dtype=F32) + F32(0.5)) - cx
    v = (np.arange(h, dtype=F32) + F32(0.5)) - cy
    with np.errstate(all="ignore"):
        return (u[None, :] * d) / fx, (v[:, None] * d) / fy, d


def color_bytes(v) -> np.ndarray:
    """clamp(rint(v), 0, 255) as uint8: ties to even, NaN gives 0"""
    with np.errstate(invalid="ignore"):
        r = np.rint(np.asarray(v, dtype=F32))
        return np.clip(np.where(np.isnan(r), F32(0), r), 0, 255).astype(np.uint8)


def sample_indices(n_out: int, n_in: int) -> np.ndarray:
    """the nearest sample of an axis of n_in values for each of n_out positions: ((2 i + 1) * n_in) // (2 * n_out)"""
    return ((2 * np.arange(n_out, dtype=np.int64) + 1) * n_in) // (2 * n_out)


def keep_mask_host(depth, depth_range=(0.0, math.inf), edge_thr=0.05, stride=1) -> np.ndarray:
    """the pixels of a depth map the point cloud keeps: valid (finite, lo < Z < hi), not a flying pixel (no valid in-frame
    4-neighbour Zn with |Z - Zn| > edge_thr * min(Z, Zn); edge_thr <= 0: no filter; neighbours at full resolution) and on the
    stride grid (y % stride == 0 and x % stride == 0)"""
    d = np.ascontiguousarray(depth, dtype=F32)
    valid = _valid_depth(d, depth_range)
    keep = valid.copy()
    thr = F32(edge_thr)
    if thr > 0:
        for a, b in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))), ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
            with np.errstate(all="ignore"):
                edge = valid[a] & valid[b] & (np.abs(d[a] - d[b]) > thr * np.minimum(d[a], d[b]))
            keep[a] &= ~edge
            keep[b] &= ~edge
    grid = np.zeros_like(keep)
    grid[::int(stride), ::int(stride)] = True
    return keep & grid


def pointcloud_host(depth, image, intrinsics, depth_range=(0.0, math.inf), edge_thr=0.05, stride=1) -> np.ndarray:
    """The specification of ``ops.pointcloud_pack`` for one frame: depth [h, w], image [3, hi, wi] (any size; nearest sample by
    ``sample_indices``, byte = ``color_bytes(v * 255)``), intrinsics fx, fy, cx, cy of the depth map's grid -> the kept pixels'
    vertices in row-major pixel order, a ``PLY_VERTEX`` array [N] (``.tobytes()``: the 15 N bytes of the cloud)"""
    if int(stride) < 1:
        raise ValueError(f"stride {stride} < 1")
    X, Y, Z = backproject_host(depth, intrinsics)
    img = np.asarray(image, dtype=F32)
    h, w = Z.shape
    keep = keep_mask_host(Z, depth_range, edge_thr, stride)
    ys, xs = np.nonzero(keep)  # row-major
    sy, sx = sample_indices(h, img.shape[1])[ys], sample_indices(w, img.shape[2])[xs]
    out = np.empty((ys.size,), dtype=PLY_VERTEX)
    out["x"], out["y"], out["z"] = X[ys, xs], Y[ys, xs], Z[ys, xs]
    for c, name in enumerate(("red", "green", "blue")):
        with np.errstate(all="ignore"):
            out[name] = color_bytes(img[c, sy, sx] * F32(255))
    return out


def normal_map_host(depth, intrinsics, depth_range=(0.0, math.inf)) -> np.ndarray:
    """The specification of ``ops.normal_rows`` for one frame -> uint8 [h, w, 3].  P = (X, Y, Z); Px = P[y, x + 1] - P[y, x - 1]
    where both neighbours are valid and in frame, else the one-sided difference with the one that is (P[y, x + 1] - P or
    P - P[y, x - 1]), else no normal; Py likewise along y.  n = cross(Px, Py) / sqrt((nx nx + ny ny) + nz nz), negated where
    (nx X + ny Y) + nz Z > 0; a zero or non-finite length or a non-finite component gives no normal.  RGB =
    ``color_bytes((n * 0.5 + 0.5) * 255)``, (0, 0, 0) for invalid pixels and pixels without a normal."""
    X, Y, Z = backproject_host(depth, intrinsics)
    P = np.stack([X, Y, Z])  # [3, h, w]
    valid = _valid_depth(Z, depth_range)

    def diff(axis):
        nxt, prv = np.roll(P, -1, axis=axis), np.roll(P, 1, axis=axis)  # (the wrapped border is masked below)
        v_nxt, v_prv = np.roll(valid, -1, axis=axis - 1), np.roll(valid, 1, axis=axis - 1)
        edge = [slice(None), slice(None)]
        edge[axis - 1] = -1
        v_nxt[tuple(edge)] = False
        edge[axis - 1] = 0
        v_prv[tuple(edge)] = False
        with np.errstate(all="ignore"):
            g = np.where(v_nxt & v_prv, nxt - prv, np.where(v_nxt, nxt - P, P - prv))
        return g, v_nxt | v_prv

    (ux, uy, uz), has_x = diff(2)
    (vx, vy, vz), has_y = diff(1)
    with np.errstate(all="ignore"):
        nx, ny, nz = uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = valid & has_x & has_y & np.isfinite(length) & (length > 0)
        nx, ny, nz = nx / length, ny / length, nz / length
        ok &= np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz)
        flip = ((nx * X + ny * Y) + nz * Z) > 0
        rgb = np.stack([color_bytes((np.where(flip, -c, c) * F32(0.5) + F32(0.5)) * F32(255)) for c in (nx, ny, nz)], axis=-1)
    rgb[~ok] = 0
    return rgb


def ply_header(n: int) -> bytes:
    """the fixed header of a cloud of n vertices"""
    return (f"ply\nformat binary_little_endian 1.0\nelement vertex {int(n)}\nproperty float x\nproperty float y\nproperty float z\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode("ascii")


def ply_bytes(n: int, vertex_bytes) -> bytes:
    """the PLY file of n vertices: the header, then the first 15 n bytes of ``vertex_bytes`` (``PLY_VERTEX`` records)"""
    body = memoryview(vertex_bytes).cast("B")[:PLY_VERTEX.itemsize * int(n)]
    if len(body) != PLY_VERTEX.itemsize * int(n):
        raise ValueError(f"ply_bytes: {n} vertices need {PLY_VERTEX.itemsize * int(n)} bytes, got {len(body)}")
    return ply_header(n) + bytes(body)


def mesh_faces_host(depth, depth_range=(0.0, math.inf), edge_thr=0.05, stride=1) -> np.ndarray:
    """The specification of the faces of ``ops.mesh_pack`` for one frame -> '<i4' [M, 3], indices into the vertices of
    ``pointcloud_host`` (the rank of a kept pixel in row-major order).  Grid node (gy, gx) is pixel (gy * stride, gx * stride);
    cell (gy, gx), gy + 1 < gh and gx + 1 < gw, has the corners a = (gy, gx), b = (gy, gx + 1), c = (gy + 1, gx), d = (gy + 1, gx + 1).
    Two kept corners are joined when edge_thr <= 0 or not (|Zp - Zq| > edge_thr * min(Zp, Zq)) -- the flying-pixel test's fp32
    operations.  Four corners kept: the diagonal a-d if |Za - Zd| <= |Zb - Zc|, else b-c; three: the diagonal whose two ends are
    kept; fewer: no face.  With a-d the candidates are (a, c, d) then (a, d, b), with b-c (a, c, b) then (b, c, d); a candidate is
    a face when its three corners are kept and its three edges are joined.  Cells in row-major order, the first candidate first.
    With x right, y down, z forward every face looks at the camera: cross(P1 - P0, P2 - P0) has negative z on a fronto-parallel
    plane."""
    s = int(stride)
    if s < 1:
        raise ValueError(f"stride {stride} < 1")
    d = np.ascontiguousarray(depth, dtype=F32)
    keep = keep_mask_host(d, depth_range, edge_thr, s)
    index = np.where(keep, np.cumsum(keep.reshape(-1), dtype=np.int64).reshape(keep.shape) - 1, -1)[::s, ::s]
    z = d[::s, ::s]
    if min(index.shape) < 2:
        return np.zeros((0, 3), dtype="<i4")
    corner = dict(a=(slice(None, -1), slice(None, -1)), b=(slice(None, -1), slice(1, None)), c=(slice(1, None), slice(None, -1)),
                  d=(slice(1, None), slice(1, None)))
    i = {n: index[c] for n, c in corner.items()}
    zc = {n: z[c] for n, c in corner.items()}
    kept = {n: v >= 0 for n, v in i.items()}
    thr = F32(edge_thr)

    def joined(p, q):
        if not thr > 0:
            return kept[p] & kept[q]
        with np.errstate(all="ignore"):
            return kept[p] & kept[q] & ~(np.abs(zc[p] - zc[q]) > thr * np.minimum(zc[p], zc[q]))

    def face(p, q, r):
        return joined(p, q) & joined(q, r) & joined(p, r), np.stack([i[p], i[q], i[r]], axis=-1)

    with np.errstate(all="ignore"):
        four = kept["a"] & kept["b"] & kept["c"] & kept["d"]
        ad = np.where(four, np.abs(zc["a"] - zc["d"]) <= np.abs(zc["b"] - zc["c"]), kept["a"] & kept["d"])
    emit, faces = [], []
    for with_ad, with_bc in (("acd", "acb"), ("adb", "bcd")):  # the first and the second candidate of a cell
        (ok_ad, tri_ad), (ok_bc, tri_bc) = face(*with_ad), face(*with_bc)
        emit.append(np.where(ad, ok_ad, ok_bc))
        faces.append(np.where(ad[..., None], tri_ad, tri_bc))
    emit, faces = np.stack(emit, axis=-1), np.stack(faces, axis=-2)  # [gh - 1, gw - 1, 2], [gh - 1, gw - 1, 2, 3]
    return np.ascontiguousarray(faces[emit], dtype="<i4")  # (boolean indexing walks cells row-major, then the candidates)


PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])  # 13 bytes, packed: the list length (3), then the vertex indices


def mesh_face_records(faces) -> np.ndarray:
    """'<i4' [M, 3] -> the ``PLY_FACE`` records [M] (``.tobytes()``: the 13 M bytes of the face element)"""
    f = np.asarray(faces, dtype="<i4").reshape(-1, 3)
    out = np.empty((f.shape[0],), dtype=PLY_FACE)
    out["n"], out["v"] = 3, f
    return out


def mesh_ply_header(n: int, m: int) -> bytes:
    """the fixed header of a mesh of n vertices and m faces: the cloud's up to its last property, then the face element"""
    head = ply_header(n)
    end = b"end_header\n"
    assert head.endswith(end)
    return head[:-len(end)] + f"element face {int(m)}\nproperty list uchar int vertex_indices\n".encode("ascii") + end


def mesh_ply_bytes(n: int, vertex_bytes, m: int, face_bytes) -> bytes:
    """the PLY file of a mesh: the header, the first 15 n bytes of ``vertex_bytes`` (``PLY_VERTEX`` records: the body of the
    cloud's file), then the first 13 m bytes of ``face_bytes`` (``PLY_FACE`` records)"""
    verts = memoryview(vertex_bytes).cast("B")[:PLY_VERTEX.itemsize * int(n)]
    faces = memoryview(face_bytes).cast("B")[:PLY_FACE.itemsize * int(m)]
    if len(verts) != PLY_VERTEX.itemsize * int(n) or len(faces) != PLY_FACE.itemsize * int(m):
        raise ValueError(f"mesh_ply_bytes: {n} vertices and {m} faces need {PLY_VERTEX.itemsize * int(n)} + {PLY_FACE.itemsize * int(m)} bytes, "
                         f"got {len(verts)} + {len(faces)}")
    return mesh_ply_header(n, m) + bytes(verts) + bytes(faces)


# ------------------------------------------------------------------------------------------------------------------
# adaptive mesh export: the host specification of ``ops.mesh_adaptive_pack`` (csrc/mesh_adaptive.hip equals it byte for byte).
# A right-triangulated irregular network over the pixel grid: the longest-edge-bisection hierarchy of blocks of ``block`` x
# ``block`` cells, cut where one per-vertex map, ``required``, says so.  The map is closed under the hierarchy (a required child
# vertex makes its parent required), which is what keeps the mesh free of T-junctions.
#   grid       vertices are pixels; kept = keep_mask_host(stride 1); the grid is padded to whole blocks, Hp = B ceil((h - 1) / B) + 1,
#              with vertices that are neither kept nor smooth
#   smooth(v)  v is kept and every 8-neighbour inside the frame is kept and joined to v (mesh_faces_host's joined)
#   hierarchy  block (y0, x0) has the corners A = (y0, x0), B' = (y0, x0 + B), C = (y0 + B, x0), D = (y0 + B, x0 + B) and the roots
#              (D, A, C), (A, D, B'); a triangle (a, b, c) has the hypotenuse a-b, the apex c, the midpoint m = (a + b) / 2 and the
#              children (c, a, m), (b, c, m); after 2 log2 B bisections the legs are one pixel long (the finest triangles)
#   vertex     not a block corner, hh = 2^min(tz(y), tz(x)): y / hh and x / hh both odd: a centre, whose hypotenuse is the diagonal
#              of its 2hh-square through the centre of the enclosing 4hh-square (the block's main diagonal for 2hh = B), whose
#              apexes are the other two corners and whose child vertices are the axial neighbours at hh; one odd: an edge midpoint,
#              hypotenuse ends at +-hh along the odd axis, apexes at +-hh along the other, child vertices the diagonal neighbours
#              at hh / 2; what falls outside the padded grid does not exist
#   required   m is not smooth, or a hypotenuse end or an existing apex is not kept, or an existing child vertex is required, or
#              (m and both ends kept) s = Za + Zb, p = Zm s, q = (Za Zb) 2, |p - q| > T p in fp32: the depth at m differs from
#              the harmonic mean of the ends -- a flat 3-D triangle's depth there -- by more than T, relative, along the ray
#   faces      blocks row-major, roots and children in the order above; a triangle above the finest is a face iff its midpoint is
#              not required, else it splits; a finest triangle is a face iff its corners are kept and its edges joined
#   vertices   the kept pixels a face references, in row-major pixel order
# ------------------------------------------------------------------------------------------------------------------
def mesh_adaptive_arguments(tolerance, block):
    """-> (T as a Python float holding a float32, B as an int), checked: T finite and >= 0, B a power of two in [2, 64]"""
    try:
        t, b = float(F32(tolerance)), int(block)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"mesh tolerance {tolerance!r} / block {block!r}: a finite number >= 0 and a power of two in [2, 64]") from None
    if not (math.isfinite(t) and t >= 0.0):
        raise ValueError(f"mesh tolerance {tolerance}: finite and >= 0")
    if b != block or b < 2 or b > 64 or b & (b - 1):
        raise ValueError(f"mesh block {block}: a power of two in [2, 64]")
    return t, b


def _adaptive_required(z, kept, smooth, T, B):
    """the ``required`` map of the padded grid (z, kept, smooth: [Hp, Wp]); block corners are left False"""
    Hp, Wp = kept.shape
    R = ~smooth
    R[::B, ::B] = False

    def geo(zm, za, zb, k):
        with np.errstate(all="ignore"):
            p = zm * (za + zb)
            q = (za * zb) * F32(2)
            return k & (np.abs(p - q) > T * p)

    def edges(R, kept, z, hh):
        """the edge midpoints at hh whose odd axis is the second one (the others: the same on the transposed views)"""
        n0 = R.shape[0]
        m = (slice(0, n0, 2 * hh), slice(hh, None, 2 * hh))
        a, b = (slice(0, n0, 2 * hh), slice(0, -1, 2 * hh)), (slice(0, n0, 2 * hh), slice(2 * hh, None, 2 * hh))
        r = R[m] | ~kept[a] | ~kept[b] | geo(z[m], z[a], z[b], kept[m] & kept[a] & kept[b])
        apex = ~kept[hh::2 * hh, hh::2 * hh]  # the rows between the edges' rows
        r[1:] |= apex
        r[:-1] |= apex
        if hh >= 2:
            c = R[hh // 2::hh, hh // 2::hh]
            c = c[:, 0::2] | c[:, 1::2]
            r[:-1] |= c[0::2]
            r[1:] |= c[1::2]
        R[m] = r

    for lg in range(B.bit_length() - 1):
        hh = 1 << lg
        edges(R, kept, z, hh)
        edges(R.T, kept.T, z.T, hh)
        m = (slice(hh, None, 2 * hh), slice(hh, None, 2 * hh))
        tl, tr = (slice(0, -1, 2 * hh), slice(0, -1, 2 * hh)), (slice(0, -1, 2 * hh), slice(2 * hh, None, 2 * hh))
        bl, br = (slice(2 * hh, None, 2 * hh), slice(0, -1, 2 * hh)), (slice(2 * hh, None, 2 * hh), slice(2 * hh, None, 2 * hh))
        i, j = np.ogrid[0:(Hp - 1) // (2 * hh), 0:(Wp - 1) // (2 * hh)]
        main = ((i + j) % 2 == 0) | (2 * hh == B)
        corners = kept[tl] & kept[tr] & kept[bl] & kept[br]
        r = R[m] | ~corners | geo(z[m], np.where(main, z[tl], z[tr]), np.where(main, z[br], z[bl]), kept[m] & corners)
        r |= R[0:-1:2 * hh, hh::2 * hh] | R[2 * hh::2 * hh, hh::2 * hh] | R[hh::2 * hh, 0:-1:2 * hh] | R[hh::2 * hh, 2 * hh::2 * hh]
        R[m] = r
    return R


def mesh_adaptive_host(depth, depth_range=(0.0, math.inf), edge_thr=0.05, tolerance=0.01, block=32):
    """The specification of ``ops.mesh_adaptive_pack`` for one frame (the rule is in the comment above) -> (the flat pixel indices
    y * w + x of the used vertices, ascending, int64 [N]; faces '<i4' [M, 3], indices into that list).  The vertex records are
    ``pointcloud_host``'s of those pixels."""
    T, B = mesh_adaptive_arguments(tolerance, block)
    T = F32(T)
    d = np.ascontiguousarray(depth, dtype=F32)
    h, w = d.shape
    none = np.zeros((0,), dtype=np.int64), np.zeros((0, 3), dtype="<i4")
    if h < 2 or w < 2:
        return none
    L = B.bit_length() - 1
    Hp, Wp = B * (-(-(h - 1) // B)) + 1, B * (-(-(w - 1) // B)) + 1
    z = np.zeros((Hp, Wp), dtype=F32)
    kept = np.zeros((Hp, Wp), dtype=bool)
    z[:h, :w], kept[:h, :w] = d, keep_mask_host(d, depth_range, edge_thr, 1)
    thr = F32(edge_thr)

    def joined(za, zb):
        if not thr > 0:
            return np.ones(np.broadcast(za, zb).shape, dtype=bool)
        with np.errstate(all="ignore"):
            return ~(np.abs(za - zb) > thr * np.minimum(za, zb))

    smooth = kept.copy()
    zr, kr, sr = z[:h, :w], kept[:h, :w], smooth[:h, :w]
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):  # (joined is symmetric: each pair once, applied to both ends)
        a = (slice(0, h - dy), slice(max(0, -dx), w - max(0, dx)))
        b = (slice(dy, h), slice(max(0, dx), w - max(0, -dx)))
        ok = kr[a] & kr[b] & joined(zr[a], zr[b])
        sr[a] &= ok
        sr[b] &= ok
    R = _adaptive_required(z, kept, smooth, T, B)

    # the triangles, level by level: slot = the first of the 2 B^2 finest slots of its block a triangle covers (+ 2 B^2 block)
    by, bx = np.divmod(np.arange(((Hp - 1) // B) * ((Wp - 1) // B), dtype=np.int64), (Wp - 1) // B)
    c16 = lambda v: v.astype(np.int16)  # noqa: E731
    y0, x0, y1, x1 = c16(by * B), c16(bx * B), c16(by * B + B), c16(bx * B + B)
    first = np.arange(by.size, dtype=np.int64) * (2 * B * B)
    slot = np.concatenate([first, first + B * B])
    ay, ax, by_, bx_ = np.concatenate([y1, y0]), np.concatenate([x1, x0]), np.concatenate([y0, y1]), np.concatenate([x0, x1])
    cy, cx = np.concatenate([y1, y0]), np.concatenate([x0, x1])
    out_slot, out_tri = [], []
    for k in range(2 * L):
        my, mx = (ay + by_) >> 1, (ax + bx_) >> 1
        split = R[my, mx]
        leaf = ~split
        out_slot.append(slot[leaf])
        out_tri.append(np.stack([ay[leaf], ax[leaf], by_[leaf], bx_[leaf], cy[leaf], cx[leaf]], axis=-1))
        ay, ax, by_, bx_, cy, cx, my, mx, slot = (v[split] for v in (ay, ax, by_, bx_, cy, cx, my, mx, slot))
        half = (B * B) >> (k + 1)
        ay, ax, by_, bx_, cy, cx = (np.concatenate(p) for p in ((cy, by_), (cx, bx_), (ay, cy), (ax, cx), (my, my), (mx, mx)))
        slot = np.concatenate([slot, slot + half])
    face = kept[ay, ax] & kept[by_, bx_] & kept[cy, cx]
    face &= joined(z[ay, ax], z[by_, bx_]) & joined(z[by_, bx_], z[cy, cx]) & joined(z[ay, ax], z[cy, cx])
    out_slot.append(slot[face])
    out_tri.append(np.stack([ay[face], ax[face], by_[face], bx_[face], cy[face], cx[face]], axis=-1))
    slot, tri = np.concatenate(out_slot), np.concatenate(out_tri).astype(np.int64)
    if not slot.size:
        return none
    tri = tri[np.argsort(slot, kind="stable")]
    pix = tri[:, 0::2] * w + tri[:, 1::2]  # [M, 3]: every corner of a face is kept, so inside the frame
    used = np.unique(pix)
    return used, np.ascontiguousarray(np.searchsorted(used, pix), dtype="<i4")


def mesh_adaptive_vertices(depth, image, intrinsics, used, depth_range=(0.0, math.inf), edge_thr=0.05) -> np.ndarray:
    """the ``PLY_VERTEX`` records of the pixels ``used`` (``mesh_adaptive_host``): ``pointcloud_host``'s records of those pixels"""
    d = np.ascontiguousarray(depth, dtype=F32)
    keep = keep_mask_host(d, depth_range, edge_thr, 1).reshape(-1)
    rank = np.cumsum(keep, dtype=np.int64) - 1
    assert keep[used].all()
    return pointcloud_host(d, image, intrinsics, depth_range, edge_thr, 1)[rank[used]]


# ------------------------------------------------------------------------------------------------------------------
# stereo export: the host specification of the right-eye view (numpy float32 for the two rounded operations, integers after them;
# csrc/stereo.hip equals it byte for byte)
# ------------------------------------------------------------------------------------------------------------------
STEREO_LAYOUTS = ("right", "sbs", "anaglyph")


def _stereo_targets(d, fx, baseline, convergence):
    """t [h, w] int64: the target column of every source pixel, in [-1, w] (-1 and w: off the frame; NaN: -1).  k = fx * baseline,
    c = k / convergence (0 for inf), s = k / Z - c, tf = float32(x) - rint(s)"""
    h, w = d.shape
    with np.errstate(all="ignore"):
        k = F32(F32(fx) * F32(baseline))
        c = F32(0) if math.isinf(float(convergence)) else F32(k / F32(convergence))
        s = (k / d).astype(F32) - c
        tf = np.arange(w, dtype=F32)[None, :] - np.rint(s)
        return np.where(np.isnan(tf), F32(-1), np.clip(tf, F32(-1), F32(w))).astype(np.int64)


def stereo_source_host(depth, intrinsics, baseline, convergence=math.inf, depth_range=(0.0, math.inf), edge_thr=0.05):
    """The specification of ``ops.stereo_source`` for one frame -> (src, filled), int32 [h, w]: the source column every column of the
    view of a second eye ``baseline`` to the right shows (same row; the camera moves along x only).  A valid pixel x (the cloud's
    rule) lands at column t(x) = x - rint(fx * baseline / Z - fx * baseline / convergence) and covers [t(x), e], e = max(t(x),
    t(x + 1) - 1) when x + 1 is in the frame, valid and joined to x (the mesh's rule: edge_thr <= 0, or not |Z - Zn| > edge_thr *
    min(Z, Zn)), else t(x): a surface that stretches in the new view has no one-pixel cracks.  Columns outside [0, w - 1] are
    dropped.  A target column keeps the source of the smallest Z, between equal Z the smaller x: ``src``, -1 for a hole.
    ``filled``: every hole of a row takes the source of the nearest non-hole column to its left or right -- the right one when its
    winner has the larger Z (the background), the left one otherwise, the one that exists at the frame's border; a row without a
    valid pixel stays -1."""
    d = np.ascontiguousarray(depth, dtype=F32)
    h, w = d.shape
    if not float(convergence) != 0.0:  # (0 and NaN)
        raise ValueError(f"convergence {convergence}: a distance other than 0 (inf: parallel axes)")
    valid = _valid_depth(d, depth_range)
    t = _stereo_targets(d, intrinsics[0], baseline, convergence)
    thr = F32(edge_thr)
    link = valid[:, :-1] & valid[:, 1:]
    if thr > 0:
        with np.errstate(all="ignore"):
            link &= ~(np.abs(d[:, :-1] - d[:, 1:]) > thr * np.minimum(d[:, :-1], d[:, 1:]))
    e = t.copy()
    e[:, :-1] = np.where(link, np.maximum(t[:, :-1], t[:, 1:] - 1), t[:, :-1])
    q0, q1 = np.maximum(t, 0), np.minimum(e, w - 1)
    n = np.where(valid, np.maximum(q1 - q0 + 1, 0), 0).reshape(-1)  # columns every source pixel covers
    who = np.repeat(np.arange(h * w, dtype=np.int64), n)             # the source pixel of every (source, target) pair
    first = np.cumsum(n) - n
    col = q0.reshape(-1)[who] + (np.arange(who.size, dtype=np.int64) - first[who])
    tgt = (who // w) * w + col
    order = np.lexsort((who % w, d.reshape(-1)[who], tgt))           # by target, then Z, then source x
    tgt, who = tgt[order], who[order]
    win = np.ones(tgt.shape, dtype=bool)
    win[1:] = tgt[1:] != tgt[:-1]
    src = np.full((h, w), -1, dtype=np.int64)
    src.reshape(-1)[tgt[win]] = who[win] % w
    # the fill: nearest non-hole column on either side
    cols = np.arange(w, dtype=np.int64)[None, :]
    shown = src >= 0
    left = np.maximum.accumulate(np.where(shown, cols, -1), axis=1)
    right = np.minimum.accumulate(np.where(shown, cols, w)[:, ::-1], axis=1)[:, ::-1]
    has_l, has_r = left >= 0, right < w
    rows = np.arange(h)[:, None]
    src_l, src_r = src[rows, np.maximum(left, 0)], src[rows, np.minimum(right, w - 1)]
    z_l, z_r = d[rows, np.maximum(src_l, 0)], d[rows, np.maximum(src_r, 0)]
    take_r = has_r & (~has_l | (z_r > z_l))
    filled = np.where(shown, src, np.where(take_r, src_r, np.where(has_l, src_l, -1)))
    return src.astype(np.int32), filled.astype(np.int32)


def _sampled_bytes(image, h, w, ys, xs):
    """uint8 [..., 3]: ``color_bytes(img[c, sy, sx] * 255)`` of the [h, w] grid's pixels (ys, xs), the cloud's colour rule"""
    img = np.asarray(image, dtype=F32)
    sy, sx = sample_indices(h, img.shape[1])[ys], sample_indices(w, img.shape[2])[xs]
    with np.errstate(all="ignore"):
        return np.stack([color_bytes(img[c, sy, sx] * F32(255)) for c in range(3)], axis=-1)


def stereo_view_host(depth, image, intrinsics, baseline, convergence=math.inf, depth_range=(0.0, math.inf), edge_thr=0.05) -> np.ndarray:
    """the right-eye view of one frame -> uint8 [h, w, 3]: column q of row y shows the image (image [3, hi, wi], any size, the
    cloud's nearest sample and byte rule) at (y, filled[y, q]) of ``stereo_source_host``, (0, 0, 0) where that is -1"""
    _, filled = stereo_source_host(depth, intrinsics, baseline, convergence, depth_range, edge_thr)
    h, w = filled.shape
    view = _sampled_bytes(image, h, w, np.arange(h)[:, None], np.maximum(filled, 0))
    view[filled < 0] = 0
    return view


def stereo_image_host(depth, image, intrinsics, baseline, convergence=math.inf, depth_range=(0.0, math.inf), edge_thr=0.05,
                      layout="right") -> np.ndarray:
    """The specification of ``ops.stereo_rows`` for one frame.  ``layout``: 'right' -> the view [h, w, 3]; 'sbs' -> left | right
    [h, 2 w, 3], left = the image sampled to the depth map's grid with the same byte rule; 'anaglyph' -> red from left, green and
    blue from right [h, w, 3]"""
    if layout not in STEREO_LAYOUTS:
        raise ValueError(f"layout {layout!r}: one of {STEREO_LAYOUTS}")
    right = stereo_view_host(depth, image, intrinsics, baseline, convergence, depth_range, edge_thr)
    if layout == "right":
        return right
    h, w = right.shape[:2]
    left = _sampled_bytes(image, h, w, np.arange(h)[:, None], np.arange(w)[None, :])
    if layout == "sbs":
        return np.ascontiguousarray(np.concatenate([left, right], axis=1))
    return np.ascontiguousarray(np.stack([left[..., 0], right[..., 1], right[..., 2]], axis=-1))


def _stereo_options(stereo):
    """the ``stereo`` dict of ``submit_geometry`` / ``write_geometry_host`` -> (baseline, convergence, layout)"""
    unknown = set(stereo) - {"baseline", "convergence", "layout"}
    if unknown:
        raise ValueError(f"stereo: unknown keys {sorted(unknown)} (baseline, convergence, layout)")
    layout = stereo.get("layout", "right")
    if layout not in STEREO_LAYOUTS:
        raise ValueError(f"stereo layout {layout!r}: one of {STEREO_LAYOUTS}")
    return float(stereo.get("baseline", 0.065)), float(stereo.get("convergence", math.inf)), layout


# ------------------------------------------------------------------------------------------------------------------
# depth-of-field export: the host specification of the frame seen through a thin lens (numpy float32, one rounding per operation in
# the order written; csrc/bokeh.hip equals it bit for bit).
#
# A tap of weight 0 changes no bit: wgt is never negative or NaN, x + 0 = x and x + 0 * c = x for every finite c.  So the host and
# the kernel may both bound their loops by the largest m in reach: with s = float32(M + 0.5), M the largest m, an offset with
# max(|dx|, |dy|) >= ceil(s) has dist >= s >= float32(me + 0.5) and cov = 0.  This is what makes tiling legal: a tile of the kernel
# walks only the window the radii in its reach can cover, and this loop only the window the frame's radii can.
#
# The loop visits one offset per pass over the frame, (2 R + 1)^2 passes: about a second for 270 x 480 at max_radius 8, minutes for
# 2160 x 3840 at 16.  It is the specification, not a route for 4K frames.
# ------------------------------------------------------------------------------------------------------------------
BOKEH_DEFAULTS = dict(aperture=0.025, focus=None, focus_point=(0.5, 0.5), max_radius=16.0)


def bokeh_focus_host(depth, focus=None, focus_point=(0.5, 0.5), depth_range=(0.0, math.inf)):
    """-> float32: the distance in focus.  ``focus`` (finite, > 0) when given; else the map at the focus point (u, v) in [0, 1]^2,
    pixel (min(h - 1, floor(v h)), min(w - 1, floor(u w))) with u, v rounded to float32 and the products in float64; NaN when that
    pixel is not valid (finite, lo < Z < hi)"""
    d = np.ascontiguousarray(depth, dtype=F32)
    h, w = d.shape
    if focus is not None:
        zf = F32(focus)
        if not (np.isfinite(zf) and zf > 0):
            raise ValueError(f"focus {focus}: a finite distance greater than 0 (None: the focus point)")
        return zf
    u, v = (float(F32(c)) for c in focus_point)
    if not (0.0 <= u <= 1.0 and 0.0 <= v <= 1.0):
        raise ValueError(f"focus point {tuple(focus_point)} outside [0, 1]^2")
    zf = d[min(h - 1, int(math.floor(v * h))), min(w - 1, int(math.floor(u * w)))]
    return zf if bool(_valid_depth(zf, depth_range)) else F32(np.nan)


def bokeh_discs_host(depth, fx, aperture, zf, max_radius, depth_range=(0.0, math.inf)):
    """-> zk, r, m, ia float32 [h, w]: valid = finite and lo < Z < hi; zk = valid ? Z : inf; iz = valid ? 1 / Z : 0; k = (fx *
    aperture) * 0.5; r = min(max_radius, k |iz - 1 / zf|) (a NaN product gives max_radius; a NaN ``zf``: r = 0 everywhere);
    m = max(r, 0.5); ia = 1 / (m m)"""
    d = np.ascontiguousarray(depth, dtype=F32)
    valid = _valid_depth(d, depth_range)
    with np.errstate(all="ignore"):
        zk = np.where(valid, d, F32(np.inf)).astype(F32)
        if np.isnan(zf):
            r = np.zeros(d.shape, F32)
        else:
            iz = np.where(valid, F32(1) / d, F32(0)).astype(F32)
            k = F32(F32(F32(fx) * F32(aperture)) * F32(0.5))
            r = np.fmin(F32(max_radius), k * np.abs(iz - F32(F32(1) / F32(zf)))).astype(F32)
        m = np.maximum(r, F32(0.5))
        ia = (F32(1) / (m * m)).astype(F32)
    return zk, r, m, ia


def _bokeh_arguments(intrinsics, aperture, max_radius):
    fx, ap, rm = F32(np.asarray(intrinsics, dtype=np.float64).reshape(-1)[0]), F32(aperture), F32(max_radius)
    if not (np.isfinite(fx) and fx > 0):
        raise ValueError(f"intrinsics: fx {fx} is finite and positive")
    if not (np.isfinite(ap) and ap >= 0):
        raise ValueError(f"aperture {aperture}: finite and not below 0 (metres)")
    if not rm >= 0:
        raise ValueError(f"max_radius {max_radius}: not below 0 (pixels)")
    return fx, ap, rm


def bokeh_render_host(depth, image, intrinsics, aperture=0.025, focus=None, focus_point=(0.5, 0.5), max_radius=16.0,
                      depth_range=(0.0, math.inf)):
    """The specification of ``ops.bokeh_render`` for one frame -> (out float32 [3, h, w], focus float32): the frame seen through a
    thin lens of diameter ``aperture`` metres focused at ``bokeh_focus_host``'s distance, the circle of confusion capped at
    ``max_radius`` pixels.  ``image`` [3, hi, wi], any size, is sampled to the map's grid with the cloud's nearest rule; a
    non-finite colour counts as 0.  With the maps of ``bokeh_discs_host``, output p sums the taps q = p + (dx, dy) inside the frame,
    dy = -R .. R outer, dx = -R .. R inner, R = ceil(max_radius): dist = float32(sqrt(dx dx + dy dy)); own = zk_q <= zk_p or
    r_q <= r_p; (me, ie) = own ? (m_q, ia_q) : (m_p, ia_p) -- a source spreads over its own disc unless it lies behind p with the
    larger one, so a defocused background does not bleed over a sharp foreground while a defocused foreground spreads over what lies
    behind it; cov = clip((me + 0.5) - dist, 0, 1); wgt = cov ie; where wgt > 0: sw += wgt, sc[ch] += wgt c_q[ch] (a multiply,
    then an add).  out = sc / sw (sw > 0: the centre tap has cov >= 0.5).  A NaN focus (an invalid focus pixel) renders r = 0
    everywhere: the sampled image itself."""
    d = np.ascontiguousarray(depth, dtype=F32)
    h, w = d.shape
    fx, ap, rm = _bokeh_arguments(intrinsics, aperture, max_radius)
    zf = bokeh_focus_host(d, focus, focus_point, depth_range)
    zk, r, m, ia = bokeh_discs_host(d, fx, ap, zf, rm, depth_range)
    img = np.asarray(image, dtype=F32)
    c = img[:, sample_indices(h, img.shape[1])[:, None], sample_indices(w, img.shape[2])[None, :]]
    c = np.where(np.isfinite(c), c, F32(0)).astype(F32)
    R = int(math.ceil(float(rm)))
    R = min(R, int(math.ceil(float(F32(m.max() + F32(0.5))))) - 1)  # (the offsets beyond have weight 0 everywhere: see above)
    sw, sc = np.zeros((h, w), F32), np.zeros((3, h, w), F32)
    for dy in range(-R, R + 1):
        y0, y1 = max(0, -dy), min(h, h - dy)
        if y0 >= y1:
            continue
        for dx in range(-R, R + 1):
            x0, x1 = max(0, -dx), min(w, w - dx)
            if x0 >= x1:
                continue
            dist = F32(math.sqrt(dx * dx + dy * dy))
            P, Q = (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            own = (zk[Q] <= zk[P]) | (r[Q] <= r[P])
            me, ie = np.where(own, m[Q], m[P]), np.where(own, ia[Q], ia[P])
            cov = np.clip((me + F32(0.5)) - dist, F32(0), F32(1))
            wgt = (cov * ie).astype(F32)
            on = wgt > 0
            sw[P] = np.where(on, sw[P] + wgt, sw[P])
            for ch in range(3):
                sc[ch][P] = np.where(on, sc[ch][P] + wgt * c[ch][Q], sc[ch][P])
    return (sc / sw).astype(F32), F32(zf)


def bokeh_image_host(depth, image, intrinsics, aperture=0.025, focus=None, focus_point=(0.5, 0.5), max_radius=16.0,
                     depth_range=(0.0, math.inf)) -> np.ndarray:
    """The specification of ``ops.bokeh_rows`` for one frame -> uint8 [h, w, 3]: ``color_bytes(out * 255)`` of ``bokeh_render_host``
    (the stereo view's byte rule)"""
    out, _ = bokeh_render_host(depth, image, intrinsics, aperture, focus, focus_point, max_radius, depth_range)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(np.moveaxis(color_bytes(out * F32(255)), 0, -1))


def _bokeh_options(bokeh):
    """the ``bokeh`` dict of ``submit_geometry`` / ``write_geometry_host`` -> dict(aperture, focus, focus_point, max_radius)"""
    unknown = set(bokeh) - set(BOKEH_DEFAULTS)
    if unknown:
        raise ValueError(f"bokeh: unknown keys {sorted(unknown)} ({', '.join(BOKEH_DEFAULTS)})")
    opt = {**BOKEH_DEFAULTS, **bokeh}
    focus = None if opt["focus"] is None else float(opt["focus"])
    u, v = (float(c) for c in opt["focus_point"])
    return dict(aperture=float(opt["aperture"]), focus=focus, focus_point=(u, v), max_radius=float(opt["max_radius"]))


def _warn_bokeh_focus(base, focus):
    if np.isnan(focus):
        print(f"warning: {os.path.basename(base)}_bokeh.png: the focus pixel holds no valid depth; the image is written as it is", flush=True)


# ------------------------------------------------------------------------------------------------------------------
# novel-view export: the host specification of the frame seen from a camera that has moved (include/prv2.h "Novel-view export";
# numpy float32 up to the fixed-point vertex positions, integers after them; csrc/view.hip equals it bit for bit).
#
# The depth map's own mesh (``mesh_faces_host``'s cells at stride 1, "kept" read as "valid") is rasterised with a depth test.  The
# faces are walked all at once: one pass over them per offset inside a face's box of pixel centres, up to the largest box that
# occurs -- 2 x 2 passes at the identity pose, 16 x 16 at most.  A pass costs a few dozen numpy operations over every face: it is
# the specification, not a route for 4K frames.
# ------------------------------------------------------------------------------------------------------------------
VIEW_MOTIONS = ("circle", "sway", "dolly")
VIEW_DEFAULTS = dict(count=8, motion="circle", amplitude=0.05, focus=math.inf)
VIEW_MAX_COUNT = 120
VIEW_MAX_FACE = 16  # prv2_view_max_face(): the pixel centres a face's box may span in x and in y
VIEW_CHUNK = 4      # views per launch of the output stage: bounds the key workspace and the pinned staging
IDENTITY_POSE = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def view_poses(count, motion="circle", amplitude=0.05, focus=math.inf) -> np.ndarray:
    """the closed camera path of the novel-view export -> float32 [count, 12], each a row-major 3 x 4 matrix [R | t] that takes a
    point of the frame's camera (x right, y down, z forward) to view k's.  theta = 2 pi k / count; the eye e is ``amplitude`` *
    (cos, sin, 0) for 'circle', (sin, 0, 0) for 'sway', (0, 0, sin) for 'dolly'.  ``focus`` = inf: R = I (parallel axes); else the
    camera keeps looking at (0, 0, focus): f = normalise((0, 0, focus) - e), r = normalise(cross((0, 1, 0), f)), d = cross(f, r), R has
    the rows r, d, f.  t = -R e.  float64 throughout, rounded once."""
    count, amplitude, focus = int(count), float(amplitude), float(focus)
    if not 1 <= count <= VIEW_MAX_COUNT:
        raise ValueError(f"view count {count}: 1 to {VIEW_MAX_COUNT}")
    if motion not in VIEW_MOTIONS:
        raise ValueError(f"view motion {motion!r}: one of {VIEW_MOTIONS}")
    if not (math.isfinite(amplitude) and amplitude >= 0.0):
        raise ValueError(f"view amplitude {amplitude}: finite and not below 0 (metres)")
    if not focus > 0.0:  # (NaN as well)
        raise ValueError(f"view focus {focus}: a depth greater than 0 (inf: parallel axes)")
    out = np.empty((count, 3, 4), dtype=np.float64)
    for k in range(count):
        th = 2.0 * math.pi * k / count
        e = amplitude * np.array({"circle": (math.cos(th), math.sin(th), 0.0), "sway": (math.sin(th), 0.0, 0.0),
                                  "dolly": (0.0, 0.0, math.sin(th))}[motion], dtype=np.float64)
        R = np.eye(3, dtype=np.float64)
        if not math.isinf(focus):
            f = np.array((0.0, 0.0, focus)) - e
            f /= np.linalg.norm(f)
            r = np.cross((0.0, 1.0, 0.0), f)
            r /= np.linalg.norm(r)
            R = np.stack([r, np.cross(f, r), f])
        out[k, :, :3], out[k, :, 3] = R, -(R @ e)
    return out.reshape(count, 12).astype(F32)


def _view_vertices(d, intrinsics, pose, depth_range):
    """-> valid, seen bool [h, w]; ux, uy int64 [h, w] (1/16 pixel, 0 where not seen); iz float32 [h, w]: the specification's
    "camera", "pose", "project" and "fixed" steps"""
    fx, fy, cx, cy = (F32(v) for v in intrinsics)
    M = [F32(v) for v in np.asarray(pose, dtype=F32).reshape(12)]
    valid = _valid_depth(d, depth_range)
    X, Y, Z = backproject_host(d, intrinsics)
    with np.errstate(all="ignore"):
        Xc, Yc, Zc = (((M[4 * r] * X + M[4 * r + 1] * Y) + M[4 * r + 2] * Z) + M[4 * r + 3] for r in range(3))
        iz = (F32(1) / Zc).astype(F32)
        fu, fv = fx * (Xc / Zc) + cx, fy * (Yc / Zc) + cy
        seen = valid & np.isfinite(Zc) & (Zc > 0) & np.isfinite(iz) & (np.abs(fu) < F32(65536)) & (np.abs(fv) < F32(65536))
        ux = np.rint(np.where(seen, fu, F32(0)) * F32(16)).astype(np.int64)
        uy = np.rint(np.where(seen, fv, F32(0)) * F32(16)).astype(np.int64)
    return valid, seen, ux, uy, iz


def _view_keys(q, source):
    """the depth-test key: ((0xFFFFFFFF - bits(q)) << 32) | source (the smallest key wins: the largest q, then the smallest source)"""
    bits = np.ascontiguousarray(q, dtype=F32).view(np.uint32).astype(np.uint64)
    return ((np.uint64(0xFFFFFFFF) - bits) << np.uint64(32)) | source.astype(np.uint64)


def view_source_host(depth, intrinsics, pose=IDENTITY_POSE, depth_range=(0.0, math.inf), edge_thr=0.05, max_face=VIEW_MAX_FACE):
    """The specification of ``ops.view_source`` for one frame and one pose -> (src, filled int32 [h, w], iz float32 [h, w]): the
    source pixel (y * w + x) every pixel of the view shows, -1 for a hole; the same with the holes of every row filled from the
    farther side (the stereo view's rule, on the winners' 1 / Zc); and the winners' interpolated 1 / Zc, 0 for a hole.  ``pose``: 12
    floats, the row-major [R | t] of ``view_poses``.  Every seen vertex is a candidate for the pixel it falls into; every face of
    the map's mesh whose three vertices are seen, whose box spans at most ``max_face`` pixel centres each way and whose area is not
    zero is a candidate for the centres it covers, edges included, front or back.  A pixel keeps the candidate of the largest
    1 / Zc, between equal ones the smallest source index.  include/prv2.h has every operation in order."""
    d = np.ascontiguousarray(depth, dtype=F32)
    h, w = d.shape
    valid, seen, ux, uy, iz = _view_vertices(d, intrinsics, pose, depth_range)
    keys = np.full((h * w,), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    index = np.arange(h * w, dtype=np.int64).reshape(h, w)
    # points
    px, py = ux >> 4, uy >> 4
    on = seen & (px >= 0) & (px < w) & (py >= 0) & (py < h)
    np.minimum.at(keys, (py * w + px)[on], _view_keys(iz[on], index[on]))
    # faces
    if h >= 2 and w >= 2:
        corner = dict(a=(slice(None, -1), slice(None, -1)), b=(slice(None, -1), slice(1, None)), c=(slice(1, None), slice(None, -1)),
                      d=(slice(1, None), slice(1, None)))
        zc = {n: d[c] for n, c in corner.items()}
        kept = {n: valid[c] for n, c in corner.items()}
        thr = F32(edge_thr)

        def joined(p, q):
            if not thr > 0:
                return kept[p] & kept[q]
            with np.errstate(all="ignore"):
                return kept[p] & kept[q] & ~(np.abs(zc[p] - zc[q]) > thr * np.minimum(zc[p], zc[q]))

        def ok(tri):
            p, q, r = tri
            return joined(p, q) & joined(q, r) & joined(p, r) & seen[corner[p]] & seen[corner[q]] & seen[corner[r]]

        with np.errstate(all="ignore"):
            four = kept["a"] & kept["b"] & kept["c"] & kept["d"]
            ad = np.where(four, np.abs(zc["a"] - zc["d"]) <= np.abs(zc["b"] - zc["c"]), kept["a"] & kept["d"])
        per_vertex = []  # [3] of (x, y, iz, index) over the faces that exist, the two candidates of every cell
        emit = np.stack([np.where(ad, ok(t_ad), ok(t_bc)) for t_ad, t_bc in (("acd", "acb"), ("adb", "bcd"))])
        for k in range(3):
            per_vertex.append([np.stack([np.where(ad, a[corner[t_ad[k]]], a[corner[t_bc[k]]]) for t_ad, t_bc in (("acd", "acb"), ("adb", "bcd"))])[emit]
                               for a in (ux, uy, iz, index)])
        (x0, y0, i0, s0), (x1, y1, i1, s1), (x2, y2, i2, s2) = per_vertex
        A = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        bx0, bx1 = (np.minimum(np.minimum(x0, x1), x2) + 7) >> 4, (np.maximum(np.maximum(x0, x1), x2) - 8) >> 4
        by0, by1 = (np.minimum(np.minimum(y0, y1), y2) + 7) >> 4, (np.maximum(np.maximum(y0, y1), y2) - 8) >> 4
        use = (A != 0) & (bx1 - bx0 + 1 <= int(max_face)) & (by1 - by0 + 1 <= int(max_face))
        bx0, bx1, by0, by1 = np.maximum(bx0, 0), np.minimum(bx1, w - 1), np.maximum(by0, 0), np.minimum(by1, h - 1)
        use &= (bx0 <= bx1) & (by0 <= by1)
        x0, y0, i0, s0, x1, y1, i1, s1, x2, y2, i2, s2, A, bx0, bx1, by0, by1 = (
            v[use] for v in (x0, y0, i0, s0, x1, y1, i1, s1, x2, y2, i2, s2, A, bx0, bx1, by0, by1))
        if A.size:
            s, area = np.sign(A), np.abs(A).astype(F32)
            for dy in range(int((by1 - by0).max()) + 1):
                for dx in range(int((bx1 - bx0).max()) + 1):
                    px, py = bx0 + dx, by0 + dy
                    cx16, cy16 = 16 * px + 8, 16 * py + 8
                    w0 = s * ((x2 - x1) * (cy16 - y1) - (y2 - y1) * (cx16 - x1))
                    w1 = s * ((x0 - x2) * (cy16 - y2) - (y0 - y2) * (cx16 - x2))
                    w2 = s * ((x1 - x0) * (cy16 - y0) - (y1 - y0) * (cx16 - x0))
                    on = (px <= bx1) & (py <= by1) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)
                    if not on.any():
                        continue
                    f0, f1, f2 = w0[on].astype(F32), w1[on].astype(F32), w2[on].astype(F32)
                    q = ((f0 * i0[on] + f1 * i1[on]) + f2 * i2[on]) / area[on]
                    source = np.where((w0[on] >= w1[on]) & (w0[on] >= w2[on]), s0[on], np.where(w1[on] >= w2[on], s1[on], s2[on]))
                    np.minimum.at(keys, (py * w + px)[on], _view_keys(q, source))
    keys = keys.reshape(h, w)
    shown = keys != np.uint64(0xFFFFFFFFFFFFFFFF)
    src = np.where(shown, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    inv = (keys >> np.uint64(32)).astype(np.int64)  # 0xFFFFFFFF - bits(q): the larger, the farther
    q_out = np.where(shown, (np.uint64(0xFFFFFFFF) - (keys >> np.uint64(32))).astype(np.uint32).view(F32), F32(0)).astype(F32)
    # the fill: nearest shown column on either side of the view's row
    cols = np.arange(w, dtype=np.int64)[None, :]
    left = np.maximum.accumulate(np.where(shown, cols, -1), axis=1)
    right = np.minimum.accumulate(np.where(shown, cols, w)[:, ::-1], axis=1)[:, ::-1]
    has_l, has_r = left >= 0, right < w
    rows = np.arange(h)[:, None]
    l, r = np.maximum(left, 0), np.minimum(right, w - 1)
    take_r = has_r & (~has_l | (inv[rows, r] > inv[rows, l]))
    filled = np.where(shown, src, np.where(take_r, src[rows, r], np.where(has_l, src[rows, l], -1)))
    return src.astype(np.int32), filled.astype(np.int32), q_out


def view_image_host(depth, image, intrinsics, pose=IDENTITY_POSE, depth_range=(0.0, math.inf), edge_thr=0.05, max_face=VIEW_MAX_FACE) -> np.ndarray:
    """The specification of ``ops.view_rows`` for one frame and one pose -> uint8 [h, w, 3]: every pixel of the view shows the image
    (image [3, hi, wi], any size, the cloud's nearest sample and byte rule) at its ``filled`` source pixel of ``view_source_host``,
    (0, 0, 0) where that is -1"""
    _, filled, _ = view_source_host(depth, intrinsics, pose, depth_range, edge_thr, max_face)
    h, w = filled.shape
    at = np.maximum(filled, 0).astype(np.int64)
    view = _sampled_bytes(image, h, w, at // w, at % w)
    view[filled < 0] = 0
    return view


def _view_options(views):
    """the ``views`` dict of ``submit_geometry`` / ``write_geometry_host`` -> dict(count, motion, amplitude, focus), checked"""
    unknown = set(views) - set(VIEW_DEFAULTS)
    if unknown:
        raise ValueError(f"views: unknown keys {sorted(unknown)} ({', '.join(VIEW_DEFAULTS)})")
    opt = {**VIEW_DEFAULTS, **views}
    opt = dict(count=int(opt["count"]), motion=opt["motion"], amplitude=float(opt["amplitude"]), focus=float(opt["focus"]))
    view_poses(**opt)  # (the checks)
    return opt


def _no_stride_with_tolerance(stride):
    if int(stride) != 1:
        raise ValueError(f"the adaptive mesh (mesh_tolerance) has no stride: stride {stride} != 1")


def write_geometry_host(base: str, depth, image, intrinsics, depth_range=(0.0, math.inf), edge_thr=0.05, stride=1, ply=True, normals=True,
                        mesh=False, stereo=None, bokeh=None, views=None, mesh_tolerance=None, mesh_block=32):
    """the host route of ``OutputStage.submit_geometry``: <base>.ply, <base>_normal.png, <base>_mesh.ply (with ``mesh_tolerance``:
    the adaptive mesh of ``mesh_adaptive_host`` with its own vertex list, which has no stride), (``stereo``: a dict of
    baseline, convergence, layout) <base>_right.png / _sbs.png / _anaglyph.png, (``bokeh``: a dict of aperture, focus, focus_point,
    max_radius) <base>_bokeh.png and (``views``: a dict of count, motion, amplitude, focus) <base>_view_000.png ... from the host
    specification"""
    if ply or mesh:
        v = pointcloud_host(depth, image, intrinsics, depth_range, edge_thr, stride)
    if ply:
        with open(base + ".ply", "wb") as f:
            f.write(ply_bytes(v.size, v.tobytes()))
    if normals:
        write_png8(base + "_normal.png", normal_map_host(depth, intrinsics, depth_range))
    if mesh and mesh_tolerance is not None:
        _no_stride_with_tolerance(stride)
        used, tri = mesh_adaptive_host(depth, depth_range, edge_thr, mesh_tolerance, mesh_block)
        av, faces = mesh_adaptive_vertices(depth, image, intrinsics, used, depth_range, edge_thr), mesh_face_records(tri)
        with open(base + "_mesh.ply", "wb") as f:
            f.write(mesh_ply_bytes(av.size, av.tobytes(), faces.size, faces.tobytes()))
    elif mesh:
        faces = mesh_face_records(mesh_faces_host(depth, depth_range, edge_thr, stride))
        with open(base + "_mesh.ply", "wb") as f:
            f.write(mesh_ply_bytes(v.size, v.tobytes(), faces.size, faces.tobytes()))
    if stereo is not None:
        baseline, convergence, layout = _stereo_options(stereo)
        write_png8(f"{base}_{layout}.png", stereo_image_host(depth, image, intrinsics, baseline, convergence, depth_range, edge_thr, layout))
    if bokeh is not None:
        opt = _bokeh_options(bokeh)
        out, focus = bokeh_render_host(depth, image, intrinsics, depth_range=depth_range, **opt)
        _warn_bokeh_focus(base, focus)
        with np.errstate(all="ignore"):
            write_png8(base + "_bokeh.png", np.ascontiguousarray(np.moveaxis(color_bytes(out * F32(255)), 0, -1)))
    if views is not None:
        for k, pose in enumerate(view_poses(**_view_options(views))):
            write_png8(f"{base}_view_{k:03d}.png", view_image_host(depth, image, intrinsics, pose, depth_range, edge_thr))


save_geometry_host = write_geometry_host  # (the name the adaptive mesh's tests and tools use)


# ------------------------------------------------------------------------------------------------------------------
# device functions
# ------------------------------------------------------------------------------------------------------------------
_LUTS = {}


def _lut_device(cmap: str, device) -> torch.Tensor:
    key = (cmap, str(device))
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(colormap_lut(cmap)).to(device)
    return _LUTS[key]


def _frames(value: torch.Tensor) -> torch.Tensor:
    """one map [H, W] / [1, 1, H, W] -> contiguous [1, H, W]"""
    if not isinstance(value, torch.Tensor) or not value.is_cuda:
        raise ValueError("the device output stage takes GPU tensors (metrics.colorize is the host route)")
    if value.dtype != torch.float32:
        raise TypeError(f"the device output stage takes float32 maps (got {value.dtype})")
    if value.dim() < 2 or any(int(s) != 1 for s in value.shape[:-2]):
        raise ValueError(f"one map [H, W] expected (got {tuple(value.shape)})")
    return value.reshape(1, value.shape[-2], value.shape[-1]).contiguous()


@torch.no_grad()
def percentile_device(value: torch.Tensor, q, mask=None, invalid_val=-99):
    """np.percentile(value[mask], q) of one fp32 device map (``mask``: bool, True = take; without it value != invalid_val): a
    float32 scalar, or a list of them for a sequence ``q``.  Exact: the order statistics come from the radix select of
    prv2_order_stats, the interpolation is numpy's.  Percentiles 0 and 100 need one call, others a count first."""
    from . import ops
    v = _frames(value)
    seq = isinstance(q, (list, tuple, np.ndarray))
    qs = list(q) if seq else [q]
    m = None if mask is None else mask.reshape(v.shape)
    if all(float(p) in (0.0, 100.0) for p in qs):
        # rank pairs known without the count: (0, 1) and (n - 1, n - 1)
        counts, out = ops.order_stats(v, [0, 1, -1], mask=m, invalid_val=invalid_val)
        n, (s0, s1, sl) = int(counts[0]), out[0].cpu().numpy()
        if n == 0:
            res = [F32(np.nan) for _ in qs]
        else:
            res = [percentile_from_sorted(s0, s1, sl, n, p) if float(p) == 0.0 else percentile_from_sorted(sl, sl, sl, n, p) for p in qs]
    else:
        counts, _ = ops.order_stats(v, [], mask=m, invalid_val=invalid_val)
        n = int(counts[0])
        if n == 0:
            res = [F32(np.nan) for _ in qs]
        else:
            res = []
            for i in range(0, len(qs), 3):  # (at most 8 ranks per call: 2 per percentile + the largest)
                part = qs[i:i + 3]
                ranks = [r for p in part for r in percentile_ranks(n, p)[:2]] + [-1]
                s = ops.order_stats(v, ranks, mask=m, invalid_val=invalid_val)[1][0].cpu().numpy()
                res += [percentile_from_sorted(s[2 * j], s[2 * j + 1], s[-1], n, p) for j, p in enumerate(part)]
    return res if seq else res[0]


@torch.no_grad()
def colorize_device(value, vmin=None, vmax=None, cmap="turbo_r", invalid_val=-99, invalid_mask=None,
                    background_color=(128, 128, 128, 255), gamma_corrected=False, value_transform=None, vminp=2, vmaxp=95):
    """``metrics.colorize`` of one fp32 device map -> (device uint8 [H, W, 3] view of the scanline buffer, the buffer itself:
    uint8 [1, prv2_rows_bytes(H, W, 3)], whose first H * (1 + 3 W) bytes are the deflate-ready image).  RGB only (every caller
    drops colorize's alpha).  vmin / vmax given by the caller are taken as float32.  ``gamma_corrected`` and
    ``value_transform`` are not built on the device: ValueError."""
    from . import ops
    if gamma_corrected or value_transform is not None:
        raise ValueError("colorize_device: gamma_corrected / value_transform are host-only (metrics.colorize)")
    v = _frames(value)
    h, w = v.shape[1:]
    inv = None if invalid_mask is None else torch.as_tensor(invalid_mask).to(v.device).bool().reshape(v.shape)
    if vmin is None or vmax is None:
        valid = None if inv is None else ~inv
        need = ([vminp] if vmin is None else []) + ([vmaxp] if vmax is None else [])
        got = percentile_device(v, need, mask=valid, invalid_val=invalid_val)
        if vmin is None:
            vmin = got.pop(0)
        if vmax is None:
            vmax = got.pop(0)
    norm = torch.from_numpy(np.array([[F32(vmin), F32(vmax)]], dtype=F32)).to(v.device)
    rows = ops.colorize_rows(v, norm, _lut_device(cmap, v.device), invalid_mask=inv, invalid_val=invalid_val, background_rgb=background_color[:3])
    img = rows[0, :h * (1 + 3 * w)].view(h, 1 + 3 * w)[:, 1:].view(h, w, 3)
    return img, rows


class OutputStage:
    """Writer of the tester's PNG files from device maps.  ``submit_*`` enqueue the scanline kernels on a side stream (after the
    producer's current stream), copy the buffers into one of ``depth`` pinned staging slots and hand (path, IHDR, rows) to a
    pool of ``workers`` threads that wait for the copy, deflate (level 6) and write the file.  A slot is reused only after its
    files are written: the ring bounds memory and gives backpressure.  ``flush()`` waits for every file and re-raises the first
    worker exception.

    ``device_deflate``: the side stream also deflates every scanline buffer (``ops.deflate_rows``).  The main thread does not
    wait for the stream sizes: they go to pinned memory with an event, the file's writer thread waits for it, copies exactly that
    many bytes on the stage's copy stream, computes the chunk CRC and writes.  Same pixels as without it, different file bytes
    (the IDAT payload is the device encoder's zlib stream)."""

    def __init__(self, work_dir: str, workers: int = 8, depth: int = 2, device_deflate: bool = False):
        self.work_dir = work_dir
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.depth = max(1, int(depth))
        self.pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="prv2-png")
        self.device_deflate = bool(device_deflate)
        self.stream = None
        self.copy_stream = None  # device_deflate / point clouds: the writer threads' D2H copies
        self._slots = [dict(buf=None, sizes=None, ply=None, ply_n=None, mesh=None, mesh_n=None, focus=None, futures=[]) for _ in range(self.depth)]
        self._loose = []  # files queued from host rows (write_rows)
        self._next = 0
        self._error = None
        self._lock = threading.Lock()
        self.bytes_d2h = 0  # bytes copied to the host so far: packed scanlines, or compressed streams and their sizes; vertex and face records and their counts
        self.files = 0
        os.makedirs(work_dir, exist_ok=True)

    # ---- pool -----------------------------------------------------------------------------------------------------
    def _write(self, path, header, rows, event=None):
        try:
            if event is not None:
                event.synchronize()  # the D2H copy of this slot
            data = png_bytes(header, rows)
            with open(path, "wb") as f:
                f.write(data)
        except BaseException as e:  # kept for flush()
            with self._lock:
                if self._error is None:
                    self._error = e

    def _check_focus(self, base, focus, event):
        """the depth-of-field view's warning: wait for the copy of the focus distance the kernel used (pinned float32 [1])"""
        try:
            event.synchronize()
            _warn_bokeh_focus(base, float(focus[0]))
        except BaseException as e:  # kept for flush()
            with self._lock:
                if self._error is None:
                    self._error = e

    def _write_stream(self, path, header, out, k, sizes, event, host):
        """device_deflate: wait for the sizes, copy stream k's bytes into the pinned view ``host``, add the CRC, write"""
        try:
            event.synchronize()  # the deflate kernels and the copy of the sizes
            nb = int(sizes[k])
            with torch.cuda.device(out.device), torch.cuda.stream(self.copy_stream):
                out.record_stream(self.copy_stream)
                host[:nb].copy_(out[0, :nb], non_blocking=True)
                done = torch.cuda.Event()
                done.record(self.copy_stream)
            done.synchronize()
            with self._lock:
                self.bytes_d2h += nb
            data = png_bytes_from_stream(header, memoryview(host.numpy())[:nb])
            with open(path, "wb") as f:
                f.write(data)
        except BaseException as e:  # kept for flush()
            with self._lock:
                if self._error is None:
                    self._error = e

    def _write_ply(self, path, header, parts, counts, event, host):
        """a PLY file of one or two elements.  ``parts``: per element (records: device uint8 [bound], bytes per record);
        ``counts``: pinned int64, element k's record count at [k].  Wait for the counts, copy exactly each element's bytes into the
        pinned ``host`` on the copy stream, prepend ``header(*counts)``, write"""
        try:
            event.synchronize()  # the count and pack kernels and the copy of the counts
            nums = [int(counts[k]) for k in range(len(parts))]
            sizes = [size * n for (_, size), n in zip(parts, nums)]
            nb = sum(sizes)
            if nb:
                with torch.cuda.device(parts[0][0].device), torch.cuda.stream(self.copy_stream):
                    off = 0
                    for (records, _), size in zip(parts, sizes):
                        records.record_stream(self.copy_stream)
                        host[off:off + size].copy_(records[:size], non_blocking=True)
                        off += size
                    done = torch.cuda.Event()
                    done.record(self.copy_stream)
                done.synchronize()
            with self._lock:
                self.bytes_d2h += nb
            with open(path, "wb") as f:
                f.write(header(*nums))
                f.write(memoryview(host.numpy())[:nb])
        except BaseException as e:  # kept for flush()
            with self._lock:
                if self._error is None:
                    self._error = e

    def write_rows(self, path: str, w: int, h: int, bpp: int, rows, event=None, _slot=None):
        """queue one file from host scanlines (a bytes-like of h * (1 + bpp * w) bytes)"""
        self.files += 1
        fut = self.pool.submit(self._write, path, ihdr(w, h, bpp), rows, event)
        (self._loose if _slot is None else _slot["futures"]).append(fut)
        return fut

    def flush(self):
        """wait for every queued file; re-raise the first worker exception"""
        for futures in [s["futures"] for s in self._slots] + [self._loose]:
            for f in futures:
                f.result()
            del futures[:]
        with self._lock:
            err, self._error = self._error, None
        if err is not None:
            raise err

    def close(self):
        try:
            self.flush()
        finally:
            self.pool.shutdown(wait=True)

    # ---- device side ----------------------------------------------------------------------------------------------
    def _begin(self, device):
        """order the side stream after the producer's current stream and take the next staging slot"""
        if self.stream is None:
            self.stream = torch.cuda.Stream(device)
            if self.device_deflate:
                self.copy_stream = torch.cuda.Stream(device)
        self.stream.wait_stream(torch.cuda.current_stream(device))
        slot = self._slots[self._next]
        self._next = (self._next + 1) % self.depth
        for f in slot["futures"]:  # backpressure: the slot's previous files must be on disk
            f.result()
        slot["futures"] = []
        return slot

    def _stage(self, slot, jobs):
        """jobs: [(path, w, h, bpp, device rows uint8 [1, bytes])] -> one pinned buffer, one event, one pool task per file"""
        if self.device_deflate:
            return self._stage_deflate(slot, jobs)
        total = sum(int(r.shape[1]) for *_, r in jobs)
        if slot["buf"] is None or slot["buf"].numel() < total:
            slot["buf"] = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
        off, views = 0, []
        for path, w, h, bpp, r in jobs:
            n = int(r.shape[1])
            slot["buf"][off:off + n].copy_(r[0], non_blocking=True)
            views.append((path, w, h, bpp, off))
            off += n
        self.bytes_d2h += total
        ev = torch.cuda.Event()
        ev.record(self.stream)
        host = slot["buf"].numpy()
        for path, w, h, bpp, o in views:
            self.write_rows(path, w, h, bpp, memoryview(host[o:o + h * (1 + bpp * w)]), ev, slot)

    def _stage_deflate(self, slot, jobs):
        """``_stage`` with the zlib streams made on the side stream: nothing but the sizes is copied here"""
        from . import ops
        streams = [ops.deflate_rows(r, h * (1 + bpp * w)) for _, w, h, bpp, r in jobs]
        total = sum(int(o.shape[1]) for o, _ in streams)  # the bounds: room for any stream
        if slot["buf"] is None or slot["buf"].numel() < total:
            slot["buf"] = torch.empty((total,), dtype=torch.uint8, pin_memory=True)
        if slot["sizes"] is None or slot["sizes"].numel() < len(jobs):
            slot["sizes"] = torch.empty((max(8, len(jobs)),), dtype=torch.int64, pin_memory=True)
        sizes = slot["sizes"]
        sizes[:len(jobs)].copy_(torch.cat([nb for _, nb in streams]), non_blocking=True)
        self.bytes_d2h += 8 * len(jobs)
        ev = torch.cuda.Event()
        ev.record(self.stream)
        off = 0
        for k, ((path, w, h, bpp, _), (out, _)) in enumerate(zip(jobs, streams)):
            self.files += 1
            host = slot["buf"][off:off + int(out.shape[1])]
            slot["futures"].append(self.pool.submit(self._write_stream, path, ihdr(w, h, bpp), out, k, sizes, ev, host))
            off += int(out.shape[1])

    @torch.no_grad()
    def submit_frame(self, base: str, result: torch.Tensor, coarse, image_raw_shape, cmap="Spectral", percentiles=(0, 100)):
        """the files of ``Tester._emit``: <base>_uint16.png, <base>.png, <base>_edge.png and, with ``coarse`` ([1, 1, ph, pw]),
        <base>_coarse.png"""
        from . import ops
        dev = result.device
        slot = self._begin(dev)
        with torch.cuda.device(dev), torch.cuda.stream(self.stream):
            d = _frames(result)
            h, w = d.shape[1:]
            jobs = [(base + "_uint16.png", w, h, 2, ops.quantize16_rows(d, 256.0)),
                    (base + ".png", w, h, 3, colorize_device(d, cmap=cmap, vminp=percentiles[0], vmaxp=percentiles[1])[1])]
            edges = ops.binary_dilate(ops.canny(ops.depth_preprocess(d, "log"), sigma=1.0), 3)  # tester.py:99-106
            jobs.append((base + "_edge.png", w, h, 1, ops.mask_rows(edges)))
            if coarse is not None:
                ch, cw = int(image_raw_shape[0]), int(image_raw_shape[1])
                up = ops.upsample_bilinear_map(coarse.reshape(1, *coarse.shape[-2:]).float(), ch, cw)
                jobs.append((base + "_coarse.png", cw, ch, 3, colorize_device(up, cmap="Spectral", vminp=0, vmaxp=100)[1]))
            self._stage(slot, jobs)
            for t in (result, coarse):
                if t is not None:
                    t.record_stream(self.stream)

    @torch.no_grad()
    def submit_geometry(self, base: str, result: torch.Tensor, image_hr, intrinsics, depth_range=(0.0, math.inf), edge_thr=0.05, stride=1,
                        ply=True, normals=True, mesh=False, stereo=None, bokeh=None, views=None, mesh_tolerance=None, mesh_block=32):
        """the geometry of one frame, from the device map: <base>.ply (``ply``: the point cloud of ``pointcloud_host``, coloured
        from ``image_hr`` [3, Hi, Wi], a host or device tensor of any size), <base>_normal.png (``normals``: the map of
        ``normal_map_host``, through the PNG path of every other file, deflated on the device with ``device_deflate``) and
        <base>_mesh.ply (``mesh``: the cloud's vertices and the faces of ``mesh_faces_host``; with ``ply`` as well the vertex
        records are made once and feed both files).  ``intrinsics``: fx, fy, cx, cy of the RESULT's grid (``camera_intrinsics``).
        The vertex and face buffers are sized for their bounds (15 bytes per strided pixel, 26 per cell); only the frame's counts
        go to pinned memory with an event, and a file's writer thread copies exactly its 15 N (+ 13 M) bytes on the copy stream.
        ``stereo`` (a dict of baseline, convergence, layout; default 0.065, inf, 'right') adds <base>_right.png, <base>_sbs.png or
        <base>_anaglyph.png: the view of ``stereo_image_host`` coloured from ``image_hr``, through the PNG path as the normal map.
        ``bokeh`` (a dict of aperture, focus, focus_point, max_radius; default 0.025, None, (0.5, 0.5), 16) adds <base>_bokeh.png: the
        frame of ``bokeh_image_host`` through the same path; the focus distance is read on the device, and only its four bytes come
        back, for the warning of a frame whose focus pixel holds no valid depth.
        ``views`` (a dict of count, motion, amplitude, focus; default 8, 'circle', 0.05, inf) adds <base>_view_000.png ...: the frames
        of ``view_image_host`` along the camera path of ``view_poses``, rendered ``VIEW_CHUNK`` views per launch, each chunk in a
        staging slot of its own, so the depth-test keys (8 bytes per view pixel) and the pinned scanlines stay bounded.
        ``mesh_tolerance`` (with ``mesh``; ``stride`` 1) makes <base>_mesh.ply the adaptive mesh of ``mesh_adaptive_host`` in blocks
        of ``mesh_block`` cells, with its own vertex list: its records come from ``ops.mesh_adaptive_pack``, a <base>.ply of the same
        call is the cloud's as before, and the copies are again the counts and exactly 15 N + 13 M bytes."""
        from . import ops
        adaptive = mesh and mesh_tolerance is not None
        if adaptive:
            _no_stride_with_tolerance(stride)
        dev = result.device
        slot = self._begin(dev)
        if (ply or mesh) and self.copy_stream is None:
            self.copy_stream = torch.cuda.Stream(dev)
        with torch.cuda.device(dev), torch.cuda.stream(self.stream):
            d = _frames(result)
            h, w = d.shape[1:]
            jobs = []
            if normals:
                jobs.append((base + "_normal.png", w, h, 3, ops.normal_rows(d, intrinsics, depth_range)))
            if ply or mesh or stereo is not None or bokeh is not None or views is not None:
                img = torch.as_tensor(image_hr)
                if img.dim() == 4 and img.shape[0] == 1:
                    img = img[0]
                img = img.to(dev, torch.float32, non_blocking=True)
            if stereo is not None:
                baseline, convergence, layout = _stereo_options(stereo)
                jobs.append((f"{base}_{layout}.png", w * (2 if layout == "sbs" else 1), h, 3,
                             ops.stereo_rows(d, img, intrinsics, baseline, convergence, depth_range, edge_thr, layout)))
            if bokeh is not None:
                rows, focus = ops.bokeh_rows(d, img, intrinsics, depth_range=depth_range, **_bokeh_options(bokeh))
                jobs.append((base + "_bokeh.png", w, h, 3, rows))
                if slot["focus"] is None:
                    slot["focus"] = torch.empty((1,), dtype=torch.float32, pin_memory=True)
                slot["focus"].copy_(focus, non_blocking=True)
                with self._lock:
                    self.bytes_d2h += 4
                ev = torch.cuda.Event()
                ev.record(self.stream)
                slot["futures"].append(self.pool.submit(self._check_focus, base, slot["focus"], ev))
            if jobs:
                self._stage(slot, jobs)
            if views is not None:
                poses = view_poses(**_view_options(views))
                for k0 in range(0, len(poses), VIEW_CHUNK):
                    rows = ops.view_rows(d, img, intrinsics, poses[k0:k0 + VIEW_CHUNK], depth_range, edge_thr)
                    self._stage(self._begin(dev), [(f"{base}_view_{k0 + k:03d}.png", w, h, 3, rows[:, k]) for k in range(rows.shape[1])])
            if ply or mesh:
                if mesh and not adaptive:
                    verts, counts, faces, n_faces = ops.mesh_pack(d, img, intrinsics, depth_range, edge_thr, stride)
                elif ply:
                    verts, counts = ops.pointcloud_pack(d, img, intrinsics, depth_range, edge_thr, stride)
            if ply:
                if slot["ply"] is None or slot["ply"].numel() < verts.shape[1]:
                    slot["ply"] = torch.empty((int(verts.shape[1]),), dtype=torch.uint8, pin_memory=True)
                if slot["ply_n"] is None:
                    slot["ply_n"] = torch.empty((1,), dtype=torch.int64, pin_memory=True)
                slot["ply_n"].copy_(counts, non_blocking=True)
                with self._lock:
                    self.bytes_d2h += 8
                ev = torch.cuda.Event()
                ev.record(self.stream)
                self.files += 1
                slot["futures"].append(self.pool.submit(self._write_ply, base + ".ply", ply_header, [(verts[0], PLY_VERTEX.itemsize)], slot["ply_n"], ev,
                                                      slot["ply"]))
            if mesh:
                if adaptive:  # (its own vertices: ``verts`` / ``counts`` stay the cloud's for the writer of <base>.ply)
                    verts, counts, faces, n_faces = ops.mesh_adaptive_pack(d, img, intrinsics, depth_range, edge_thr, mesh_tolerance, mesh_block)
                room = int(verts.shape[1]) + int(faces.shape[1])
                if slot["mesh"] is None or slot["mesh"].numel() < room:
                    slot["mesh"] = torch.empty((room,), dtype=torch.uint8, pin_memory=True)
                    slot["mesh_n"] = torch.empty((2,), dtype=torch.int64, pin_memory=True)
                slot["mesh_n"][:1].copy_(counts, non_blocking=True)
                slot["mesh_n"][1:].copy_(n_faces, non_blocking=True)
                with self._lock:
                    self.bytes_d2h += 16
                ev = torch.cuda.Event()
                ev.record(self.stream)
                self.files += 1
                slot["futures"].append(self.pool.submit(self._write_ply, base + "_mesh.ply", mesh_ply_header,
                                                      [(verts[0], PLY_VERTEX.itemsize), (faces[0], PLY_FACE.itemsize)], slot["mesh_n"], ev, slot["mesh"]))
            result.record_stream(self.stream)
            if isinstance(image_hr, torch.Tensor) and image_hr.is_cuda:
                image_hr.record_stream(self.stream)

    @torch.no_grad()
    def submit_pseudo_label(self, base: str, depth, uncertainty, count_map, n_tiles: int, count_thr: float, cmap="magma_r"):
        """the five files of ``Tester._write_pl``"""
        from . import ops
        dev = depth.device
        slot = self._begin(dev)
        with torch.cuda.device(dev), torch.cuda.stream(self.stream):
            d, u, c = _frames(depth), _frames(uncertainty), _frames(count_map)
            h, w = d.shape[1:]
            thr = float(count_thr) * n_tiles
            # extrema of the uncertainty: of the whole map, and of the pixels enough tiles cover (u is monotone in it there, 1 elsewhere)
            _, s_all = ops.order_stats(u, [0, -1], invalid_val=float("nan"))
            n_in, s_in = ops.order_stats(u, [0, -1], invalid_val=float("nan"), gate=c, gate_thr=thr)
            lo, hi = (float(x) for x in s_all[0].cpu().numpy().astype(np.float64))
            n_in = int(n_in[0])
            in_lo, in_hi = (float(x) for x in s_in[0].cpu().numpy().astype(np.float64))

            def unit(x):
                return (x - lo) / (hi - lo) if hi > lo else 0.0
            vals = ([unit(in_lo), unit(in_hi)] if n_in > 0 else []) + ([1.0] if n_in < h * w else [])
            prm = torch.tensor([[lo, hi, thr, min(vals), max(vals)]], dtype=torch.float64).to(dev)
            r16, rgb = ops.pl_uncertainty_rows(u, c, prm, _lut_device("jet", dev))
            jobs = [(base + ".png", w, h, 3, colorize_device(d, cmap=cmap, vminp=0, vmaxp=100)[1]),
                    (base + "_uint16.png", w, h, 2, ops.quantize16_rows(d, 256.0)),
                    (base + "_uncert_uint16.png", w, h, 2, r16),
                    (base + "_uncert.png", w, h, 3, rgb),
                    (base + "_count_uint16.png", w, h, 2, ops.quantize16_rows(c, 256.0))]
            self._stage(slot, jobs)
            for t in (depth, uncertainty, count_map):
                t.record_stream(self.stream)
