#!/usr/bin/env python
"""Cost of the mesh export (--save-mesh; csrc/pointcloud.hip, patchrefinerv2_amd/output.py): one JSON line (also written to ``--out``,
default profiles/mesh_export.json).

  python tools/bench_mesh.py [--reps 10] [--maps 2] [--skip-tester] [--baseline-tree DIR --runs 3] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- steps ``4k`` (2160 x 3840) and ``1080p`` (1080 x 1920), on the synthetic depth map and image of tools/bench_geometry.py, for the mesh
  at stride 1 and stride 4; wall-clock medians per frame, no file written on either side:
    ``device_ms``   what OutputStage.submit_geometry(mesh=True) and its writer do up to the file: the kernels (vertex records, index map,
                    face count, face records), N and M to the host, the copy of exactly 15 N + 13 M bytes into pinned memory;
    ``kernels_ms``  the kernels alone; ``cloud_kernels_ms``: ops.pointcloud_pack alone, the part the cloud already pays;
    ``host_ms``     the numpy host route of the same commit (the specification, not the code under test): the fp32 map copied to the
                    host, pointcloud_host + mesh_faces_host + mesh_ply_bytes;
    ``d2h_bytes_*`` bytes copied device -> host per frame on either route; ``equal``: the two routes' bytes are the same.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over ``--maps`` synthetic images with --save
  --device-output: without and with --save-mesh, with --save-ply and both, and the mesh at stride 4; files go to a temporary directory
  (the disk is part of the figure) and are on disk when the clock stops.
- step ``baseline`` (with ``--baseline-tree DIR``, a built checkout of the commit to compare with): Tester.run maps/s of the paths this
  export does not touch -- no save, and --save --device-output --save-ply -- ``--runs`` times on this tree and on that one, in
  separate processes.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from bench_geometry import SIZES, _rates, synth  # noqa: E402
from evalbench import wall_ms  # noqa: E402

STEPS = ("4k", "1080p", "tester", "baseline", "baseline_other")


def step_size(step, reps):
    from patchrefinerv2_amd import ops, output as O
    h, w = SIZES[step]
    depth, image = synth(h, w)
    k = O.camera_intrinsics((h, w), (h, w))
    d, img = torch.from_numpy(depth).cuda()[None], torch.from_numpy(image).cuda()[None]
    res = dict(shape=[h, w])
    for stride in (1, 4):
        gh, gw = -(-h // stride), -(-w // stride)
        pinned = torch.empty((15 * gh * gw + 26 * (gh - 1) * (gw - 1),), dtype=torch.uint8, pin_memory=True)
        nm_pin = torch.empty((2,), dtype=torch.int64, pin_memory=True)

        def kernels():
            return ops.mesh_pack(d, img, k, stride=stride)

        def cloud_kernels():
            return ops.pointcloud_pack(d, img, k, stride=stride)

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

        def host():
            z = d[0].cpu().numpy()
            v = O.pointcloud_host(z, image, k, stride=stride)
            f = O.mesh_face_records(O.mesh_faces_host(z, stride=stride))
            return O.mesh_ply_bytes(v.size, v.tobytes(), f.size, f.tobytes())
        nv, nf = device()
        equal = O.mesh_ply_header(nv // 15, nf // 13) + pinned[:nv + nf].numpy().tobytes() == host()
        res[f"mesh_stride{stride}"] = dict(points=nv // 15, faces=nf // 13, device_ms=wall_ms(device, reps), kernels_ms=wall_ms(kernels, reps),
                                           cloud_kernels_ms=wall_ms(cloud_kernels, reps), host_ms=wall_ms(host, 3, warm=1),
                                           d2h_bytes_device=nv + nf + 16, d2h_bytes_host=4 * h * w, equal=bool(equal))
    return res


def step_tester(n_maps):
    dev = dict(save=True, device_output=True)
    return _rates(dict(device=dev, device_mesh=dict(dev, save_mesh=True), device_ply=dict(dev, save_ply=True),
                       device_ply_mesh=dict(dev, save_ply=True, save_mesh=True), device_mesh_stride4=dict(dev, save_mesh=True, ply_stride=4)),
                  n_maps)


def step_baseline(n_maps, runs):
    return _rates(dict(no_save={}, device_ply=dict(save=True, device_output=True, save_ply=True)), n_maps, runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maps", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3, help="--baseline-tree: timed runs per case and tree")
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--baseline-tree", default=None, help="a built checkout to compare Tester.run without the new flag with")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_export.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.baseline_tree) if a.step == "baseline_other" else ROOT)
        EB.begin_step()
        if a.step in SIZES:
            res = step_size(a.step, a.reps)
        elif a.step == "tester":
            res = step_tester(a.maps)
        else:
            res = step_baseline(a.maps, a.runs)
        return EB.end_step(res)
    steps = [s for s in STEPS if not (a.skip_tester and s == "tester") and (a.baseline_tree or not s.startswith("baseline"))]
    args = ["--reps", a.reps, "--maps", a.maps, "--runs", a.runs] + (["--baseline-tree", a.baseline_tree] if a.baseline_tree else [])
    out = EB.run_steps(__file__, steps, a.step_timeout, args)
    if "baseline" in out:
        out["baseline"] = dict(this_tree=out.pop("baseline"), other_tree=out.pop("baseline_other"))
    return EB.report(out, a.out)


if __name__ == "__main__":
    sys.exit(main())
