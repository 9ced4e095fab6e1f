#!/usr/bin/env python
"""Cost and size of the adaptive mesh export (--save-mesh --mesh-tolerance; csrc/mesh_adaptive.hip, patchrefinerv2_amd/output.py) beside
the grid mesh of --save-mesh: one JSON line (also written to ``--out``, default profiles/mesh_adaptive.json).

  python tools/bench_mesh_adaptive.py [--reps 10] [--maps 2] [--skip-tester] [--skip-deviation] [--parent-tree DIR] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- steps ``4k`` (2160 x 3840) and ``1080p`` (1080 x 1920), on the portrait scene of tools/bench_bokeh.py (a subject at 1.5 m in front of
  a background that recedes from 2 m to 12 m) with the grid-mesh bench's noise (0.01 rand) over the whole map.  Per mesh --
  ``grid_stride1`` and ``grid_stride4`` (ops.mesh_pack), ``T<tolerance>_B<block>`` for T in 0.002, 0.005, 0.01, 0.02 at B = 32 and
  B in 8, 16, 64 at T = 0.01 (ops.mesh_adaptive_pack) -- wall-clock medians per frame, no file written:
    ``vertices`` / ``faces`` / ``file_bytes``  the counts and 15 N + 13 M + the header;
    ``kernels_ms``  the op alone; ``device_ms``: with N and M to the host and the copy of exactly 15 N + 13 M bytes into pinned memory;
    ``dev_max`` / ``dev_p99`` / ``covered``  (host, numpy; not for grid_stride1, whose vertices are the pixels) the along-ray relative
                    deviation |Zs - Z| / Z of every pixel a face covers from the emitted surface -- Zs: the face's plane, inverse
                    depth affine in pixel coordinates -- its largest value and 99th percentile, and the covered share of the pixels;
    ``equal``       (adaptive meshes) the device's bytes are the numpy specification's.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over ``--maps`` synthetic images with --save
  --device-output --save-mesh, without and with --mesh-tolerance 0.01; files go to a temporary directory and are on disk when the clock
  stops.
- steps ``parent_k`` / ``this_k``, k = 0, 1, 2, alternating (with ``--parent-tree DIR``, a built checkout of the parent commit): the
  unchanged path -- Tester.run --save --device-output --save-mesh without the new flag -- on that tree and on this one.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from bench_bokeh import synth as portrait  # noqa: E402
from bench_geometry import SIZES, _rates  # noqa: E402
from evalbench import wall_ms  # noqa: E402

AB = tuple(f"{tree}_{k}" for k in range(3) for tree in ("parent", "this"))  # alternating
STEPS = ("4k", "1080p", "tester") + AB
CONFIGS = [(0.002, 32), (0.005, 32), (0.01, 32), (0.02, 32), (0.01, 8), (0.01, 16), (0.01, 64)]


def scene(h, w):
    d, image = portrait(h, w)
    return (d + 0.01 * np.random.RandomState(1).rand(h, w)).astype(np.float32), image


def surface_deviation(depth, py, px, faces, chunk=1 << 22):
    """depth [h, w]; py, px: the pixel of every vertex; faces [M, 3] -> (largest, 99th percentile of |Zs - Z| / Z over the pixels a
    face covers, the covered share of the pixels).  Zs is the depth of the face's plane at the pixel: inverse depth interpolated with
    the pixel's barycentric coordinates.  A pixel on an edge two faces share takes the larger value."""
    h, w = depth.shape
    dev = np.full((h, w), -1.0, dtype=np.float64)
    fy, fx = py[faces].astype(np.int64), px[faces].astype(np.int64)  # [M, 3]
    inv = 1.0 / depth[fy, fx].astype(np.float64)
    y0, x0 = fy.min(axis=1), fx.min(axis=1)
    bh, bw = fy.max(axis=1) - y0, fx.max(axis=1) - x0
    for sh, sw in sorted(set(zip(bh.tolist(), bw.tolist()))):
        sel = np.flatnonzero((bh == sh) & (bw == sw))
        gy, gx = (v.reshape(-1) for v in np.mgrid[0:sh + 1, 0:sw + 1])
        step = max(1, chunk // gy.size)
        for i in range(0, sel.size, step):
            s = sel[i:i + step]
            qy, qx = y0[s, None] + gy[None], x0[s, None] + gx[None]  # [F, P]
            ay, ax, by, bx, cy, cx = (v[s, j, None] for j in range(3) for v in (fy, fx))
            area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            wa = ((bx - qx) * (cy - qy) - (by - qy) * (cx - qx)) / area
            wb = ((cx - qx) * (ay - qy) - (cy - qy) * (ax - qx)) / area
            wc = 1.0 - wa - wb
            inside = (wa >= 0) & (wb >= 0) & (wc >= -1e-12)
            zs = 1.0 / (wa * inv[s, 0, None] + wb * inv[s, 1, None] + wc * inv[s, 2, None])
            z = depth[qy[inside], qx[inside]].astype(np.float64)
            np.maximum.at(dev, (qy[inside], qx[inside]), np.abs(zs[inside] - z) / z)
    got = dev[dev >= 0]
    if not got.size:
        return None, None, 0.0
    return float(got.max()), float(np.percentile(got, 99)), round(got.size / (h * w), 6)


def step_size(step, reps, deviation):
    from patchrefinerv2_amd import ops, output as O
    h, w = SIZES[step]
    depth, image = scene(h, w)
    k = O.camera_intrinsics((h, w), (h, w))
    d, img = torch.from_numpy(depth).cuda()[None], torch.from_numpy(image).cuda()[None]
    pinned = torch.empty((15 * h * w + 26 * (h - 1) * (w - 1),), dtype=torch.uint8, pin_memory=True)
    nm_pin = torch.empty((2,), dtype=torch.int64, pin_memory=True)
    res = dict(shape=[h, w])

    def measure(kernels):
        def device():
            verts, n, faces, m = kernels()
            nm_pin[:1].copy_(n, non_blocking=True)
            nm_pin[1:].copy_(m, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            nv, nf = 15 * int(nm_pin[0]), 13 * int(nm_pin[1])
            pinned[:nv].copy_(verts[0, :nv], non_blocking=True)
            pinned[nv:nv + nf].copy_(faces[0, :nf], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            return nv, nf
        nv, nf = device()
        body = pinned[:nv + nf].numpy().tobytes()
        out = dict(vertices=nv // 15, faces=nf // 13, file_bytes=len(O.mesh_ply_header(nv // 15, nf // 13)) + nv + nf,
                   kernels_ms=wall_ms(kernels, reps), device_ms=wall_ms(device, reps))
        return out, body

    def with_deviation(out, py, px, faces):
        if deviation:
            out["dev_max"], out["dev_p99"], out["covered"] = surface_deviation(depth, py, px, faces)
        return out

    for stride in (1, 4):
        out, _ = measure(lambda: ops.mesh_pack(d, img, k, stride=stride))
        if stride > 1:
            py, px = np.nonzero(O.keep_mask_host(depth, stride=stride))
            with_deviation(out, py, px, O.mesh_faces_host(depth, stride=stride))
        res[f"grid_stride{stride}"] = out
    for tol, block in CONFIGS:
        out, body = measure(lambda: ops.mesh_adaptive_pack(d, img, k, tolerance=tol, block=block))
        used, faces = O.mesh_adaptive_host(depth, tolerance=tol, block=block)
        v, rec = O.mesh_adaptive_vertices(depth, image, k, used), O.mesh_face_records(faces)
        out["equal"] = bool(body == v.tobytes() + rec.tobytes())
        res[f"T{tol:g}_B{block}"] = with_deviation(out, *np.divmod(used, w), faces)
    return res


def step_tester(n_maps):
    dev = dict(save=True, device_output=True, save_mesh=True)
    return _rates(dict(grid_mesh=dev, adaptive_mesh=dict(dev, mesh_tolerance=0.01, mesh_block=32)), n_maps)


def step_unchanged(n_maps):
    return _rates(dict(grid_mesh=dict(save=True, device_output=True, save_mesh=True)), n_maps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maps", type=int, default=2)
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--skip-deviation", action="store_true", help="leave the host's deviation measurement out of the size steps")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: the unchanged path (--save-mesh alone) on both trees")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_adaptive.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.parent_tree) if a.step.startswith("parent") else ROOT)
        EB.begin_step()
        if a.step in SIZES:
            return EB.end_step(step_size(a.step, a.reps, not a.skip_deviation))
        return EB.end_step(step_tester(a.maps) if a.step == "tester" else step_unchanged(a.maps))
    steps = [s for s in STEPS if not (a.skip_tester and s == "tester") and (a.parent_tree or s not in AB)]
    args = ["--reps", a.reps, "--maps", a.maps] + (["--skip-deviation"] if a.skip_deviation else []) + (
        ["--parent-tree", a.parent_tree] if a.parent_tree else [])
    return EB.report(EB.run_steps(__file__, steps, a.step_timeout, args), a.out)


if __name__ == "__main__":
    sys.exit(main())
