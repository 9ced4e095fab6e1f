#!/usr/bin/env python
"""Cost of the novel-view export (--save-views; csrc/view.hip, patchrefinerv2_amd/output.py): one JSON line (also written to ``--out``,
default profiles/view_export.json).

  python tools/bench_views.py [--reps 10] [--maps 2] [--skip-tester] [--baseline-tree DIR --runs 3] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- steps ``4k`` (2160 x 3840) and ``1080p`` (1080 x 1920), on the portrait scene of tools/bench_bokeh.py (a subject 1.5 m away in
  front of a background that recedes from 2 m to 12 m; a camera of a 60 degree field of view), for the identity pose and for view 1 of
  8 of ``circle`` at 0.05 m and at 0.5 m (parallel axes); wall-clock medians per view, one view per call, no file written:
    ``clear_ms`` / ``raster_ms`` / ``resolve_ms``  each of the three kernels of ops.view_rows alone (prv2_view_stages);
    ``kernels_ms``     the three together;
    ``device_ms``      what OutputStage.submit_geometry(views=...) does per view up to the writer: the kernels and the copy of the
                       scanline buffer into pinned memory;
    ``atomics``        the 64-bit minima the raster kernel issues on the key buffer (counted by a torch restatement of the face
                       boxes), ``atomics_per_pixel``, ``gatomics_s`` and ``atomic_gbytes_s`` (8 bytes each) over ``raster_ms``;
    ``copy_same_bytes_ms`` / ``copy_gbytes_s``     a torch device copy of as many bytes as the minima carry, on the same box;
    ``holes``          the share of the view's pixels no candidate reaches (before the fill).
- step ``host``: the numpy host route once at 270 x 480 (view_image_host, circle at 0.05 m) and whether the device's bytes equal it.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over ``--maps`` synthetic images with --save
  --device-output: without and with --save-views 8; files go to a temporary directory (the disk is part of the figure).
- steps ``baseline`` / ``baseline_other`` (with ``--baseline-tree DIR``, a built checkout of the commit to compare with): Tester.run
  maps/s of the paths this export does not touch -- no save, and --save --device-output -- once per process, ``--runs`` times
  alternating between this tree and that one.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from bench_bokeh import synth  # noqa: E402
from bench_geometry import SIZES, _rates  # noqa: E402
from evalbench import wall_ms  # noqa: E402

STEPS = ("4k", "1080p", "host", "tester", "baseline", "baseline_other")
EDGE_THR = 0.05


def cases():
    from patchrefinerv2_amd import output as O
    return dict(identity=np.array(O.IDENTITY_POSE, dtype=np.float32), circle_0p05=O.view_poses(8, "circle", 0.05)[1],
                circle_0p5=O.view_poses(8, "circle", 0.5)[1])


def count_minima(d, k, pose, thr, cap):
    """the candidates of one view -> (points, face pixels): the specification's vertices and face boxes restated with torch on the
    device (float32; a statistic, not the oracle: that is view_source_host)"""
    h, w = d.shape
    fx, fy, cx, cy = (float(v) for v in k)
    m = [float(v) for v in pose]
    ys, xs = torch.meshgrid(torch.arange(h, device=d.device, dtype=torch.float32), torch.arange(w, device=d.device, dtype=torch.float32),
                            indexing="ij")
    valid = torch.isfinite(d) & (d > 0)
    X, Y = ((xs + 0.5) - cx) * d / fx, ((ys + 0.5) - cy) * d / fy
    xc, yc, zc = (((m[4 * r] * X + m[4 * r + 1] * Y) + m[4 * r + 2] * d) + m[4 * r + 3] for r in range(3))
    fu, fv = fx * (xc / zc) + cx, fy * (yc / zc) + cy
    seen = valid & torch.isfinite(zc) & (zc > 0) & torch.isfinite(1 / zc) & (fu.abs() < 65536) & (fv.abs() < 65536)
    ux = torch.where(seen, torch.round(fu * 16), torch.zeros_like(fu)).to(torch.int64)
    uy = torch.where(seen, torch.round(fv * 16), torch.zeros_like(fv)).to(torch.int64)
    px, py = ux >> 4, uy >> 4
    points = int((seen & (px >= 0) & (px < w) & (py >= 0) & (py < h)).sum())
    corner = dict(a=(slice(None, -1), slice(None, -1)), b=(slice(None, -1), slice(1, None)), c=(slice(1, None), slice(None, -1)),
                  d=(slice(1, None), slice(1, None)))

    def joined(p, q):
        zp, zq = d[corner[p]], d[corner[q]]
        return valid[corner[p]] & valid[corner[q]] & ~((zp - zq).abs() > thr * torch.minimum(zp, zq))

    four = valid[corner["a"]] & valid[corner["b"]] & valid[corner["c"]] & valid[corner["d"]]
    ad = torch.where(four, (d[corner["a"]] - d[corner["d"]]).abs() <= (d[corner["b"]] - d[corner["c"]]).abs(), valid[corner["a"]] & valid[corner["d"]])
    total = 0
    for t_ad, t_bc in (("acd", "acb"), ("adb", "bcd")):
        ok = torch.where(ad, *(joined(t[0], t[1]) & joined(t[1], t[2]) & joined(t[0], t[2]) & seen[corner[t[0]]] & seen[corner[t[1]]]
                               & seen[corner[t[2]]] for t in (t_ad, t_bc)))
        (x0, y0), (x1, y1), (x2, y2) = [[torch.where(ad, u[corner[t_ad[i]]], u[corner[t_bc[i]]])[ok] for u in (ux, uy)] for i in range(3)]
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        bx0, bx1 = (torch.minimum(torch.minimum(x0, x1), x2) + 7) >> 4, (torch.maximum(torch.maximum(x0, x1), x2) - 8) >> 4
        by0, by1 = (torch.minimum(torch.minimum(y0, y1), y2) + 7) >> 4, (torch.maximum(torch.maximum(y0, y1), y2) - 8) >> 4
        use = (area != 0) & (bx1 - bx0 + 1 <= cap) & (by1 - by0 + 1 <= cap)
        bx0, bx1, by0, by1 = bx0.clamp(min=0), bx1.clamp(max=w - 1), by0.clamp(min=0), by1.clamp(max=h - 1)
        use &= (bx0 <= bx1) & (by0 <= by1)
        x0, y0, x1, y1, x2, y2, area, bx0, bx1, by0, by1 = (v[use] for v in (x0, y0, x1, y1, x2, y2, area, bx0, bx1, by0, by1))
        if not area.numel():
            continue
        s = torch.sign(area)
        for dy in range(int((by1 - by0).max()) + 1):
            for dx in range(int((bx1 - bx0).max()) + 1):
                qx, qy = 16 * (bx0 + dx) + 8, 16 * (by0 + dy) + 8
                w0 = s * ((x2 - x1) * (qy - y1) - (y2 - y1) * (qx - x1))
                w1 = s * ((x0 - x2) * (qy - y2) - (y0 - y2) * (qx - x2))
                w2 = s * ((x1 - x0) * (qy - y0) - (y1 - y0) * (qx - x0))
                total += int(((bx0 + dx <= bx1) & (by0 + dy <= by1) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0)).sum())
    return points, total


def step_size(step, reps):
    from patchrefinerv2_amd import ops, output as O
    lib = ops.L.load()
    h, w = SIZES[step]
    depth, image = synth(h, w)
    k = O.camera_intrinsics((h, w), (h, w))
    d, img = torch.from_numpy(depth).cuda()[None], torch.from_numpy(image).cuda()[None]
    pinned = torch.empty((lib.prv2_rows_bytes(h, w, 3),), dtype=torch.uint8, pin_memory=True)
    res = dict(shape=[h, w], edge_thr=EDGE_THR, key_bytes=8 * h * w, d2h_bytes_per_view=int(pinned.numel()))
    for name, pose in cases().items():
        p = torch.from_numpy(pose).cuda()[None]

        def kernels():
            return ops.view_rows(d, img, k, p, edge_thr=EDGE_THR)

        def device():
            pinned.copy_(kernels()[0, 0], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        r = dict(kernels_ms=wall_ms(kernels, reps), device_ms=wall_ms(device, reps))
        kernels()
        for stage, mask in (("clear_ms", 1), ("raster_ms", 2), ("resolve_ms", 4)):
            assert lib.prv2_view_stages(mask) == 7
            try:
                r[stage] = wall_ms(kernels, reps)
            finally:
                lib.prv2_view_stages(7)
        points, faces = count_minima(d[0], k, pose, EDGE_THR, int(lib.prv2_view_max_face()))
        n = points + faces
        src = ops.view_source(d, k, p, edge_thr=EDGE_THR)[0]
        a, b = torch.empty((n,), dtype=torch.int64, device="cuda"), torch.empty((n,), dtype=torch.int64, device="cuda")
        copy_ms = wall_ms(lambda: b.copy_(a), reps)
        r.update(atomics=n, atomics_per_pixel=round(n / (h * w), 3), gatomics_s=round(n / r["raster_ms"] / 1e6, 2),
                 atomic_gbytes_s=round(8 * n / r["raster_ms"] / 1e6, 1), copy_same_bytes_ms=copy_ms, copy_gbytes_s=round(8 * n / copy_ms / 1e6, 1),
                 holes=round(float((src < 0).float().mean()), 5))
        res[name] = r
    return res


def step_host():
    from patchrefinerv2_amd import ops, output as O
    h, w = 270, 480
    depth, image = synth(h, w)
    k = O.camera_intrinsics((h, w), (h, w))
    pose = cases()["circle_0p05"]
    rows = ops.view_rows(torch.from_numpy(depth).cuda(), torch.from_numpy(image).cuda(), k, pose, edge_thr=EDGE_THR)
    got = rows[0, 0].cpu().numpy()[:h * (1 + 3 * w)].reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3)
    t0 = time.perf_counter()
    want = O.view_image_host(depth, image, k, pose, edge_thr=EDGE_THR)
    return dict(shape=[h, w], host_ms=round((time.perf_counter() - t0) * 1e3, 1), equal=bool(np.array_equal(got, want)))


def step_tester(n_maps):
    dev = dict(save=True, device_output=True)
    return _rates(dict(device=dev, device_views8=dict(dev, save_views=8)), n_maps)


def step_baseline(n_maps):
    return _rates(dict(no_save={}, device=dict(save=True, device_output=True)), n_maps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maps", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3, help="--baseline-tree: timed runs per case and tree, alternating between the trees")
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--skip-sizes", action="store_true")
    ap.add_argument("--baseline-tree", default=None, help="a built checkout to compare Tester.run without the new flag with")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_export.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.baseline_tree) if a.step == "baseline_other" else ROOT)
        EB.begin_step()
        if a.step in SIZES:
            res = step_size(a.step, a.reps)
        elif a.step == "host":
            res = step_host()
        elif a.step == "tester":
            res = step_tester(a.maps)
        else:
            res = step_baseline(a.maps)
        return EB.end_step(res)
    steps = [s for s in STEPS if not s.startswith("baseline") and not (a.skip_tester and s == "tester") and not (a.skip_sizes and s in SIZES + ("host",))]
    args = ["--reps", a.reps, "--maps", a.maps] + (["--baseline-tree", a.baseline_tree] if a.baseline_tree else [])
    out = EB.run_steps(__file__, steps, a.step_timeout, args)
    if a.baseline_tree:
        runs = [EB.run_steps(__file__, ["baseline", "baseline_other"], a.step_timeout, args) for _ in range(a.runs)]
        names = [c for c in runs[0]["baseline"] if c in ("no_save", "device")]
        out["baseline"] = {tree: {**{c: v for c, v in runs[0][key].items() if c not in names}, **{c: [r[key][c] for r in runs] for c in names}}
                           for tree, key in (("this_tree", "baseline"), ("other_tree", "baseline_other"))}
    return EB.report(out, a.out)


if __name__ == "__main__":
    sys.exit(main())
