#!/usr/bin/env python
"""Cost of the KITTI and ScanNet dataset evaluation (datasets.KittiDataset / ScanNetDataset): one JSON line (also written to ``--out``,
default profiles/kitti_scannet_eval.json).

  python tools/bench_kitti_scannet_eval.py [--reps 20] [--maps 4] [--skip-tester] [--parent-tree DIR] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- step ``metrics``, per frame, at KITTI's size (375 x 1242 source, 352 x 1216 kb-crop window) and at two ScanNet sizes (depth 480 x 640
  beside a 968 x 1296 image; depth and image 1440 x 1920):
    ``new_ms.item``         H2D of the image's and the depth PNG's bytes from pinned memory, ops.u8_image and ops.depth16_gt;
    ``new_ms.depth16_gt``   the decode kernel alone;
    ``new_ms.get_metrics``  the dataset's get_metrics on the device (KITTI: one fused scoring pass inside the Garg crop; ScanNet: the
                            log-depth Canny of the ground truth, its 7 x 7 dilation, one fused pass over three pixel sets);
    ``host_ms``             the host route of the same commit, which is the specification: PIL's crop / resize(NEAREST), the numpy
                            decode with get_boundaries (``item``; the image's crop and / 255 included) and metrics.compute_metrics
                            (``get_metrics``; ScanNet: metrics.edge_split_masks and three calls);
  whether the two routes' depth, boundary and region are equal and the largest relative difference of their metrics.  Wall-clock
  medians of ``--reps`` calls (host: one call) with a device synchronisation at each end; ``*_alloc_bytes``: device bytes ALLOCATED
  per call.
- steps ``tester_kitti`` / ``tester_scannet``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over a synthetic tree of
  that dataset, with ground truth and with it dropped from the items.
- steps ``plain<i>`` / ``parent<i>`` (with ``--parent-tree DIR``, a built checkout of the parent commit): Tester.run maps/s over a folder
  of images without ground truth -- a run that does not touch the new datasets -- with this tree's package and with the parent's,
  three runs each, alternating.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from evalbench import alloc_bytes, wall_ms  # noqa: E402

MIN_DEPTH, MAX_DEPTH = 1e-3, 80
KB = (352, 1216)
KITTI_SRC = (375, 1242)
SCANNET_SIZES = (((480, 640), (968, 1296)), ((1440, 1920), (1440, 1920)))  # (depth, image)
PAIRS = 3
STEPS = ("metrics", "tester_kitti", "tester_scannet") + tuple(f"{tag}{i}" for i in range(1, PAIRS + 1) for tag in ("plain", "parent"))


def image_scene(shape, k=0):
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([90 + 60 * (x > (0.3 + 0.01 * k) * w), 80 + 90 * (y > 0.55 * h), 100 + 50 * np.sin(x / 37.0) * np.cos(y / 53.0)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


def kitti_scene(shape, k=0):
    """-> (metres float32, the depth PNG's uint16 samples: sparse returns of a road scene, none in the top third)"""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 6.0 + 60.0 * (1.0 - y / h) ** 2 + 0.002 * x
    d[(y > 0.55 * h) & (y < 0.8 * h) & (x > (0.2 + 0.01 * k) * w) & (x < (0.3 + 0.01 * k) * w)] = 9.0
    raw = np.round(d * 256).astype(np.uint16)
    raw[np.random.RandomState(k).rand(h, w) > 0.35] = 0
    raw[:h // 3] = 0
    return d.astype(np.float32), raw


def scannet_scene(shape, k=0):
    """-> the depth PNG's uint16 samples (millimetres): a tilted floor, a nearer wall and a pillar, a few zeros"""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 3200.0 + 900.0 * x / w + 500.0 * y / h
    wall = x < (0.3 + 0.01 * k) * w
    d[wall] = 1500.0 + 300.0 * y[wall] / h
    d[(y >= 0.66 * h) & (x >= 0.62 * w) & (x < 0.87 * w)] = 2100.0
    raw = np.round(d).astype(np.uint16)
    raw[::97, ::89] = 0
    return raw


def _rel(a, b):
    return max(abs(a[k] - b[k]) / max(1e-12, abs(b[k])) for k in b if not (np.isnan(a[k]) and np.isnan(b[k])))


def _case(ds, img, raw, out_hw, divisor, decode_kw, host_item, host_metrics, pred, reps, with_region):
    """one size: the device route's timings, the host route's (one call each) and whether the two agree"""
    from patchrefinerv2_amd import metrics as M, ops
    pins = [torch.from_numpy(np.ascontiguousarray(a)).pin_memory() for a in (img, raw)]

    def item():
        i, r = (p.cuda(non_blocking=True) for p in pins)
        return (ops.u8_image(i, swap_rb=False),) + ops.depth16_gt(r, out_hw, divisor, **decode_kw)
    image, depth, boundary = item()
    samples = pins[1].cuda()
    gt = depth[None, None]

    def new():
        return ds.get_metrics(gt, pred, disp_gt_edges=boundary)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h_img, h_depth, h_boundary = host_item()
    host_item_ms = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    h_metrics, h_region = host_metrics(h_depth, h_boundary, pred.cpu())
    host_metrics_ms = round((time.perf_counter() - t0) * 1e3, 1)
    a = new()
    equal = dict(image=bool(np.array_equal(image.cpu().numpy(), h_img)),
                 depth=bool(np.array_equal(depth.cpu().numpy().view(np.uint32), h_depth.view(np.uint32))),
                 boundary=bool(np.array_equal(boundary.cpu().numpy(), h_boundary.astype(np.uint8))))
    if with_region:
        equal["region_pixels_differing"] = int((M.edge_split_masks_device(depth, 7).cpu().numpy().astype(bool) != h_region).sum())
    return dict(source=list(raw.shape), output=list(out_hw), metric_keys=len(a), equal=equal,
                new_ms=dict(item=wall_ms(item, reps), depth16_gt=wall_ms(lambda: ops.depth16_gt(samples, out_hw, divisor, **decode_kw), reps),
                            get_metrics=wall_ms(new, reps)),
                host_ms=dict(item=host_item_ms, get_metrics=host_metrics_ms),
                new_alloc_bytes=dict(item=alloc_bytes(item), get_metrics=alloc_bytes(new)),
                max_rel_diff_new_vs_host=float(f"{_rel(a, {k: float(v) for k, v in h_metrics.items()}):.3e}"))


def step_metrics(reps):
    from PIL import Image
    from patchrefinerv2_amd import metrics as M
    from patchrefinerv2_amd.tester import KittiDataset, ScanNetDataset
    out = {}
    # KITTI
    ds = KittiDataset.__new__(KittiDataset)
    ds.min_depth, ds.max_depth = MIN_DEPTH, MAX_DEPTH
    dense, raw = kitti_scene(KITTI_SRC)
    img = image_scene(KITTI_SRC)
    top, left = int(KITTI_SRC[0] - KB[0]), int((KITTI_SRC[1] - KB[1]) / 2)
    box = (left, top, left + KB[1], top + KB[0])
    pred = torch.from_numpy(np.ascontiguousarray(dense[top:top + KB[0]:2, left:left + KB[1]:2]) * np.float32(1.1))[None, None].cuda()

    def kitti_item():  # kitti_dataset.py:114-142, :155, :203
        image = np.asarray(Image.fromarray(img).crop(box), dtype=np.float32) / 255.0
        depth = np.asarray(Image.fromarray(raw).crop(box), dtype=np.float32) / 256.0
        return np.ascontiguousarray(image.transpose(2, 0, 1)), depth, M.get_boundaries(depth, th=1, dilation=0)

    def kitti_metrics(depth, boundary, p):
        with np.errstate(invalid="ignore"):
            return M.compute_metrics(torch.from_numpy(depth)[None, None], p.clone(), disp_gt_edges=boundary, min_depth_eval=MIN_DEPTH,
                                     max_depth_eval=MAX_DEPTH, garg_crop=True, eigen_crop=False, dataset="kitti"), None
    out["kitti"] = _case(ds, img[top:top + KB[0], left:left + KB[1]], raw, KB, 256.0, dict(window=(top, left)), kitti_item, kitti_metrics, pred, reps,
                         False)
    # ScanNet
    ds = ScanNetDataset.__new__(ScanNetDataset)
    ds.min_depth, ds.max_depth = MIN_DEPTH, MAX_DEPTH
    for depth_hw, image_hw in SCANNET_SIZES:
        raw = scannet_scene(depth_hw)
        img = image_scene(image_hw)
        xx = np.linspace(0.9, 1.2, image_hw[1] // 2, dtype=np.float32)
        pred = torch.from_numpy(scannet_scene((image_hw[0] // 2, image_hw[1] // 2)).astype(np.float32) / np.float32(1000) * xx)[None, None].cuda()

        def scannet_item():  # scannet_dataset.py:109-137, :188
            image = np.asarray(Image.fromarray(img).convert("RGB")).astype(np.float32).copy() / 255.0
            depth = np.asarray(Image.fromarray(raw).resize((image_hw[1], image_hw[0]), Image.NEAREST)).astype(np.float32).copy() / 1000.0
            return np.ascontiguousarray(image.transpose(2, 0, 1)), depth, M.get_boundaries(depth, th=1, dilation=0)

        def scannet_metrics(depth, boundary, p):  # scannet_dataset.py:221-243
            region = M.edge_split_masks(depth)
            kw = dict(disp_gt_edges=boundary, min_depth_eval=MIN_DEPTH, max_depth_eval=MAX_DEPTH, garg_crop=False, eigen_crop=False, dataset="")
            res = {}
            for pre, mask in (("edge_", torch.from_numpy(region)), ("noedge_", torch.from_numpy(~region)), ("", None)):
                res.update({pre + k: v for k, v in M.compute_metrics(torch.from_numpy(depth)[None, None], p.clone(), additional_mask=mask, **kw).items()})
            return res, region
        out[f"scannet_{depth_hw[0]}x{depth_hw[1]}_to_{image_hw[0]}x{image_hw[1]}"] = _case(
            ds, img, raw, image_hw, 1000.0, dict(nearest=True), scannet_item, scannet_metrics, pred, reps, True)
    return out


def write_kitti_tree(root, n):
    from PIL import Image
    from patchrefinerv2_amd.output import write_png16
    lines = []
    for k in range(n):
        rel_img, rel_depth = f"2011_09_26/drive_0002/image_02/data/{k:010d}.png", f"drive_0002/proj_depth/groundtruth/image_02/{k:010d}.png"
        for p in (os.path.join(root, "raw", rel_img), os.path.join(root, "depth", rel_depth)):
            os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(image_scene(KITTI_SRC, k)).save(os.path.join(root, "raw", rel_img))
        write_png16(os.path.join(root, "depth", rel_depth), kitti_scene(KITTI_SRC, k)[1])
        lines.append(f"{rel_img} {rel_depth} 721.5377\n")
    split = os.path.join(root, "eigen_test.txt")
    with open(split, "w") as f:
        f.writelines(lines)
    return split


def write_scannet_tree(root, n, depth_hw, image_hw):
    from PIL import Image
    from patchrefinerv2_amd.output import write_png16
    lines = []
    for k in range(n):
        img = os.path.join(root, "data", "1ada7a0617", "iphone", "rgb", f"frame_{k:06d}.png")
        depth = os.path.join(root, "data", "1ada7a0617", "iphone", "render_depth", f"frame_{k:06d}.png")
        for p in (img, depth):
            os.makedirs(os.path.dirname(p), exist_ok=True)
        Image.fromarray(image_scene(image_hw, k)).save(img)
        write_png16(depth, scannet_scene(depth_hw, k))
        lines.append(f"{img} {depth}\n")
    split = os.path.join(root, "nvs_sem_val.txt")
    with open(split, "w") as f:
        f.writelines(lines)
    return split


def step_tester(kind, n_maps):
    from patchrefinerv2_amd.tester import KittiDataset, ScanNetDataset
    w, model = EB.workload_model()
    tc = dict(degree=1.0, network_process_size=[384, 512])
    with tempfile.TemporaryDirectory() as root:
        if kind == "kitti":
            frame = KB
            ds = KittiDataset("infer", root, write_kitti_tree(root, n_maps), tc, MIN_DEPTH, MAX_DEPTH)
        else:
            depth_hw, frame = SCANNET_SIZES[1]
            ds = ScanNetDataset("infer", write_scannet_tree(root, n_maps, depth_hw, frame), tc, MIN_DEPTH, MAX_DEPTH)
        w = dict(w, raw=list(frame))  # the frames are the dataset's size
        out, keys = EB.gt_pair_maps_s(model, ds, w, n_maps)
        ds.close()
    return dict(workload=EB.WORKLOAD, maps=n_maps, frame=list(frame), metric_keys=keys, **out)


def step_plain(n_maps):
    """Tester.run over a folder of images without ground truth: nothing of the new datasets runs"""
    from patchrefinerv2_amd.tester import ImageDataset
    w, model = EB.workload_model()
    with tempfile.TemporaryDirectory() as root:
        for k in range(n_maps):
            np.save(os.path.join(root, f"{k:05d}.npy"), np.random.default_rng(k).integers(0, 256, tuple(w["raw"]) + (3,), dtype=np.uint8))
        ds = ImageDataset(root, image_resolution=w["raw"], min_depth=MIN_DEPTH, max_depth=80)
        maps_s, res, _ = EB.timed_maps_s(model, ds, w, n_maps)
        assert "metrics" not in res[0]
    return dict(maps=n_maps, maps_s=maps_s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--maps", type=int, default=4)
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: the plain Tester.run from its package too")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kitti_scannet_eval.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.parent_tree) if a.step.startswith("parent") else ROOT)
        EB.begin_step()
        if a.step == "metrics":
            return EB.end_step(step_metrics(a.reps))
        return EB.end_step(step_tester(a.step[len("tester_"):], a.maps) if a.step.startswith("tester_") else step_plain(a.maps))
    steps = [s for s in STEPS if s == "metrics" or not a.skip_tester]
    if not a.parent_tree:  # (the alternating pairs need both trees)
        steps = [s for s in steps if not s.startswith(("plain", "parent"))]
    out = EB.run_steps(__file__, steps, a.step_timeout, ["--reps", a.reps, "--maps", a.maps] + (["--parent-tree", a.parent_tree] if a.parent_tree else []))
    if a.parent_tree and not a.skip_tester:  # the two trees' rows: every run, and whether each tree's median lies inside the other's spread
        rows = {tag: [out.pop(f"{tag}{i}")["maps_s"] for i in range(1, PAIRS + 1)] for tag in ("plain", "parent")}
        inside = all(min(rows[b]) <= sorted(rows[a_])[PAIRS // 2] <= max(rows[b]) for a_, b in (("plain", "parent"), ("parent", "plain")))
        out["without_the_dataset"] = dict(workload=EB.WORKLOAD, maps=a.maps, this_commit_maps_s=rows["plain"], parent_maps_s=rows["parent"],
                                          medians_inside_each_others_spread=inside)
    return EB.report(out, a.out)


if __name__ == "__main__":
    sys.exit(main())
