#!/usr/bin/env python
"""Cost of the geometry export (--save-ply / --save-normals; csrc/pointcloud.hip, patchrefinerv2_amd/output.py): one JSON line (also
written to ``--out``, default profiles/geometry_export.json).

  python tools/bench_geometry.py [--reps 10] [--maps 2] [--skip-tester] [--baseline-tree DIR --runs 3] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- steps ``4k`` (2160 x 3840) and ``1080p`` (1080 x 1920), on one synthetic depth map with a step edge and an image of the same size, for
  the point cloud at stride 1 and stride 4 and for the normal map; wall-clock medians per frame, no file written on either side:
    ``device_ms``   what OutputStage.submit_geometry and its writer do up to the file: the kernels, the count to the host, the copy of
                    exactly 15 N bytes (the normal map: its scanlines) into pinned memory;
    ``kernels_ms``  the kernels alone;
    ``host_ms``     the numpy host route of the same commit (the specification, not the code under test): the fp32 map copied to the
                    host, pointcloud_host + ply_bytes (normal_map_host);
    ``d2h_bytes_*`` bytes copied device -> host per frame on either route; ``equal``: the two routes' bytes are the same.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over ``--maps`` synthetic images: no save, --save
  --device-output, the same with --save-ply, with --save-normals, and the host route (--save) with both flags; files go to a temporary
  directory (the disk is part of the figure) and are on disk when the clock stops.
- step ``baseline`` (with ``--baseline-tree DIR``, a built checkout of the commit to compare with): Tester.run maps/s without the new
  flags -- no save, and --save --device-output -- ``--runs`` times on this tree and on that one, in separate processes.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from evalbench import wall_ms  # noqa: E402

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
STEPS = ("4k", "1080p", "tester", "baseline", "baseline_other")


def synth(h, w, seed=0):
    """a depth map with a slope, a disc in front (step edges: flying pixels) and noise; an image of the same size"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    rs = np.random.RandomState(seed)
    d = 5.0 + 30.0 * (x / w) - 3.0 * (np.hypot(x - w * 0.6, y - h * 0.5) < h * 0.2) + 0.5 * np.sin(y / 37.0) + 0.01 * rs.rand(h, w)
    return d.astype(np.float32), rs.rand(3, h, w).astype(np.float32)


def step_size(step, reps):
    from patchrefinerv2_amd import ops, output as O
    h, w = SIZES[step]
    depth, image = synth(h, w)
    k = O.camera_intrinsics((h, w), (h, w))
    d, img = torch.from_numpy(depth).cuda()[None], torch.from_numpy(image).cuda()[None]
    res = dict(shape=[h, w])
    for stride in (1, 4):
        pinned = torch.empty((15 * -(-h // stride) * -(-w // stride),), dtype=torch.uint8, pin_memory=True)
        n_pin = torch.empty((1,), dtype=torch.int64, pin_memory=True)

        def kernels():
            return ops.pointcloud_pack(d, img, k, stride=stride)

        def device():
            verts, counts = kernels()
            n_pin.copy_(counts, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            nb = 15 * int(n_pin[0])
            pinned[:nb].copy_(verts[0, :nb], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            return nb

        def host():
            v = O.pointcloud_host(d[0].cpu().numpy(), image, k, stride=stride)
            return O.ply_bytes(v.size, v.tobytes())
        nb = device()
        equal = O.ply_header(nb // 15) + pinned[:nb].numpy().tobytes() == host()
        res[f"ply_stride{stride}"] = dict(points=nb // 15, device_ms=wall_ms(device, reps), kernels_ms=wall_ms(kernels, reps),
                                          host_ms=wall_ms(host, 3, warm=1), d2h_bytes_device=nb + 8, d2h_bytes_host=4 * h * w, equal=bool(equal))
    rows_pin = torch.empty((ops.L.load().prv2_rows_bytes(h, w, 3),), dtype=torch.uint8, pin_memory=True)

    def n_kernels():
        return ops.normal_rows(d, k)

    def n_device():
        rows_pin.copy_(n_kernels()[0], non_blocking=True)
        torch.cuda.current_stream().synchronize()

    def n_host():
        return O.normal_map_host(d[0].cpu().numpy(), k)
    n_device()
    got = rows_pin.numpy()[:h * (1 + 3 * w)].reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3)
    res["normals"] = dict(device_ms=wall_ms(n_device, reps), kernels_ms=wall_ms(n_kernels, reps), host_ms=wall_ms(n_host, 3, warm=1),
                          d2h_bytes_device=int(rows_pin.numel()), d2h_bytes_host=4 * h * w, equal=bool(np.array_equal(got, n_host())))
    return res


def _image_folder(root, n, shape=(270, 480)):
    from patchrefinerv2_amd.tester import ImageDataset
    imgs = os.path.join(root, "imgs")
    os.makedirs(imgs)
    for i in range(n):
        np.save(os.path.join(imgs, f"f{i}.npy"), np.random.RandomState(i).rand(*shape, 3).astype(np.float32))
    return imgs, ImageDataset


def _rates(cases, n_maps, runs=1):
    """Tester.run maps/s of every case (name -> RunnerInfo keywords) on the flagship workload: a warm-up run, then ``runs`` timed ones"""
    from patchrefinerv2_amd.tester import RunnerInfo
    w, model = EB.workload_model()
    out = {}
    with tempfile.TemporaryDirectory() as root:
        imgs, ImageDataset = _image_folder(root, n_maps)
        ds = ImageDataset(imgs, image_resolution=w["raw"])
        for name, kw in cases.items():
            vals = []
            for r in range(runs):
                info = RunnerInfo(rank=0, world_size=1, work_dir=os.path.join(root, f"{name}_{r}"), output_workers=8, **kw)
                vals.append(EB.timed_maps_s(model, ds, w, n_maps, info=info)[0])
            out[name] = vals[0] if runs == 1 else vals
    return dict(workload=EB.WORKLOAD, maps=n_maps, mode=w["mode"], **out)


def step_tester(n_maps):
    dev = dict(save=True, device_output=True)
    return _rates(dict(no_save={}, device=dev, device_ply=dict(dev, save_ply=True), device_normals=dict(dev, save_normals=True),
                       device_ply_stride4=dict(dev, save_ply=True, ply_stride=4),
                       host_ply_normals=dict(save=True, save_ply=True, save_normals=True)), n_maps)


def step_baseline(n_maps, runs):
    return _rates(dict(no_save={}, device=dict(save=True, device_output=True)), n_maps, runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maps", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3, help="--baseline-tree: timed runs per case and tree")
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--baseline-tree", default=None, help="a built checkout to compare Tester.run without the new flags with")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_export.json"))
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
