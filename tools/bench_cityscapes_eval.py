#!/usr/bin/env python
"""Cost of the Cityscapes dataset evaluation (datasets.CityScapesDataset): one JSON line (also written to ``--out``, default
profiles/cityscapes_eval.json).

  python tools/bench_cityscapes_eval.py [--reps 20] [--maps 4] [--skip-tester] [--parent-tree DIR] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

Sizes are Cityscapes': image, disparity and colour segmentation map 1024 x 2048, prediction 1024 x 2048.
- step ``metrics``, per frame:
    ``new_ms.item``         H2D of the three files' bytes from pinned memory, ops.u8_image and ops.cityscapes_gt (depth, boundary and the
                            float segmentation map in one pass);
    ``new_ms.get_metrics``  CityScapesDataset.get_metrics on the device (ops.seg_canny, the log-depth Canny of the ground truth and of
                            the prediction, ops.image_edge_region, ops.cityscapes_masks, one fused scoring pass, the boundary metrics);
    ``host_ms``             the host specification route of the same commit: the numpy decode and metrics.seg_canny / extract_edges /
                            cityscapes_masks / compute_metrics / compute_boundary_metrics (the image-edge region comes from the device:
                            its host restatement lives with the tests);
  whether the two routes' masks are equal and the largest relative difference of their metrics.  Wall-clock medians of ``--reps``
  calls (host: one call) with a device synchronisation at each end; ``*_alloc_bytes``: device bytes ALLOCATED per frame.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over a synthetic Cityscapes tree, with ground truth
  and with it dropped from the items.
- steps ``plain<i>`` / ``parent<i>`` (with ``--parent-tree DIR``, a built checkout of the parent commit): Tester.run maps/s over a folder
  of images without ground truth -- a run that does not touch the new dataset -- with this tree's package and with the parent's,
  three runs each, alternating.
"""
from __future__ import annotations

import argparse
import json
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

MIN_DEPTH, MAX_DEPTH = 1e-3, 250
SHAPE = (1024, 2048)
BASELINE, FX = 0.209313, 2262.52
COLOURS = dict(sky=(70, 130, 180), building=(70, 70, 70), road=(128, 64, 128), person=(220, 20, 60), car=(0, 0, 142), pole=(153, 153, 153))
PAIRS = 3
STEPS = ("metrics", "tester") + tuple(f"{tag}{i}" for i in range(1, PAIRS + 1) for tag in ("plain", "parent"))


def scene(shape, k=0):
    """-> (image uint8 [h, w, 3], segmentation colours uint8 [h, w, 3], disparity samples uint16 [h, w]): a street of flat classes
    with straight, diagonal and curved boundaries and thin poles; disparity falls with the row and steps at the objects"""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    seg = np.empty((h, w, 3), np.uint8)
    seg[:] = COLOURS["road"]
    seg[y < 0.35 * h] = COLOURS["sky"]
    seg[(x > (0.6 + 0.01 * k) * w) & (y < 0.6 * h)] = COLOURS["building"]
    seg[(y > 0.4 * h) & (x * h + y * w < 0.5 * h * w)] = COLOURS["person"]
    seg[np.hypot(y - 0.62 * h, x - 0.4 * w) < 0.12 * h] = COLOURS["car"]
    for px in (0.15, 0.52, 0.83):
        seg[int(0.2 * h):int(0.7 * h), int(px * w):int(px * w) + 3] = COLOURS["pole"]
    disp = 4.0 + 40.0 * (y / h) ** 2
    for name, add in (("building", 3.0), ("person", 30.0), ("car", 18.0), ("pole", 9.0)):
        disp = disp + add * (seg == np.array(COLOURS[name], np.uint8)).all(-1)
    raw = (np.round(disp * 256) + 1).astype(np.uint16)
    raw[(seg == np.array(COLOURS["sky"], np.uint8)).all(-1)] = 0
    raw[::97, ::89] = 0
    img = seg.astype(np.float32) * 0.6 + 40 + 12 * np.sin(x / 37.0)[..., None] * np.cos(y / 53.0)[..., None]
    return np.clip(img, 0, 255).astype(np.uint8), seg, raw


def decode_host(raw, seg, factor):
    """cityscapes_dataset.py:153-174, :300 in numpy -> (depth float32, boundary float32)"""
    from patchrefinerv2_amd import metrics as M
    d = raw.astype(np.float32)
    d[d > 0] = (d[d > 0] - 1) / 256
    with np.errstate(divide="ignore"):
        depth = np.nan_to_num(np.float32(factor) / d, posinf=0., neginf=0., nan=0.).astype(np.float32)
    h, w = depth.shape
    depth[-h // 4:, :] = -1.
    depth[:, :w // 16] = -1.
    depth[:, -w // 16:] = -1.
    depth[np.logical_and(seg[:, :, 0] == 70, seg[:, :, 1] == 130)] = 0
    return depth, M.get_boundaries(depth, th=1, dilation=0)


def step_metrics(reps):
    from patchrefinerv2_amd import metrics as M, ops
    from patchrefinerv2_amd.tester import CityScapesDataset
    img, seg, raw = scene(SHAPE)
    factor = float(np.float32(BASELINE * FX))
    pins = [torch.from_numpy(a).pin_memory() for a in (img, raw, seg)]
    ds = CityScapesDataset.__new__(CityScapesDataset)
    ds.min_depth, ds.max_depth = MIN_DEPTH, MAX_DEPTH

    def item():
        i, r, s = (p.cuda(non_blocking=True) for p in pins)
        return (ops.u8_image(i, swap_rb=False),) + ops.cityscapes_gt(r, s, factor)
    image, depth, boundary, seg_f = item()
    gt = depth[None, None]
    xx = torch.arange(SHAPE[1], device="cuda")
    pred = (torch.where(gt > 0, gt, torch.full_like(gt, 20.0)) * (1 + 0.05 * torch.sin(xx / 11.0))).contiguous()

    def new():
        return ds.get_metrics(gt, pred, boundary, seg_image=seg_f, image_hr=image)

    def masks_new():
        region = ops.image_edge_region(image, *SHAPE, frac=0.05)
        return ops.cityscapes_masks(ops.seg_canny(seg_f), M.extract_edges_device(depth, "log"), region) + (region,)

    masks = {}

    def host():
        d, b = decode_host(raw, seg, factor)
        region = ops.image_edge_region(image, *SHAPE, frac=0.05).cpu().numpy()  # (no host restatement in the package)
        edge, flatten = M.cityscapes_masks(M.seg_canny(seg.transpose(2, 0, 1).astype(np.float32)), M.extract_edges(d, "log"), region)
        masks.update(edge=edge, flatten=flatten, depth=d)
        g, p = torch.from_numpy(d)[None, None], pred.cpu()
        with np.errstate(invalid="ignore"):
            out = dict(M.compute_metrics(g, p.clone(), disp_gt_edges=b, additional_mask=torch.from_numpy(flatten), min_depth_eval=MIN_DEPTH,
                                         max_depth_eval=MAX_DEPTH, garg_crop=False, eigen_crop=False, dataset=""))
        out.update(M.compute_boundary_metrics(edge, M.extract_edges(p, "log"), (d > MIN_DEPTH) & (d < MAX_DEPTH)))
        return {k: float(v) for k, v in out.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b = host()
    host_ms = round((time.perf_counter() - t0) * 1e3, 1)
    a = new()
    e, f, region = masks_new()
    agree = max(abs(a[k] - b[k]) / max(1e-12, abs(b[k])) for k in b if not (np.isnan(a[k]) and np.isnan(b[k])))
    valid = (masks["depth"] > MIN_DEPTH) & (masks["depth"] < MAX_DEPTH)
    return dict(shape=list(SHAPE), metric_keys=len(a), depth_equal=bool(np.array_equal(depth.cpu().numpy(), masks["depth"])),
                edge_pixels=int(masks["edge"].sum()), flatten_share_of_valid=round(float((masks["flatten"] & valid).sum() / max(1, valid.sum())), 4),
                edge_region_share=round(float(region.float().mean()), 4),
                mask_pixels_differing=dict(edge=int((e.cpu().numpy().astype(bool) != masks["edge"]).sum()),
                                           flatten=int((f.cpu().numpy().astype(bool) != masks["flatten"]).sum())),
                new_ms=dict(item=wall_ms(item, reps), seg_canny=wall_ms(lambda: ops.seg_canny(seg_f), reps), masks=wall_ms(masks_new, reps),
                            get_metrics=wall_ms(new, reps)),
                host_ms=host_ms, new_alloc_bytes=dict(item=alloc_bytes(item), get_metrics=alloc_bytes(new)),
                max_rel_diff_new_vs_host=float(f"{agree:.3e}"))


def step_tester(n_maps):
    from PIL import Image
    from patchrefinerv2_amd.output import write_png16
    from patchrefinerv2_amd.tester import CityScapesDataset
    w, model = EB.workload_model()
    w = dict(w, raw=list(SHAPE))  # the frames are Cityscapes' size
    with tempfile.TemporaryDirectory() as root:
        lines = []
        for kind in ("leftImg8bit", "disparity", "gtFine", "camera"):
            os.makedirs(os.path.join(root, kind, "val", "ulm"))
        for k in range(n_maps):
            stem = f"val/ulm/ulm_{k:06d}_000019"
            img, seg, raw = scene(SHAPE, k)
            Image.fromarray(img).save(os.path.join(root, f"leftImg8bit/{stem}_leftImg8bit.png"))
            Image.fromarray(seg).save(os.path.join(root, f"gtFine/{stem}_gtFine_color.png"))
            write_png16(os.path.join(root, f"disparity/{stem}_disparity.png"), raw)
            with open(os.path.join(root, f"camera/{stem}_camera.json"), "w") as f:
                json.dump(dict(extrinsic=dict(baseline=BASELINE), intrinsic=dict(fx=FX + k)), f)
            lines.append(f"leftImg8bit/{stem}_leftImg8bit.png disparity/{stem}_disparity.png\n")
        split = os.path.join(root, "val.txt")
        with open(split, "w") as f:
            f.writelines(lines)
        ds = CityScapesDataset("infer", split, dict(degree=1.0, network_process_size=[384, 512]), MIN_DEPTH, MAX_DEPTH, data_root=root,
                               with_seg_map=True)
        out, keys = EB.gt_pair_maps_s(model, ds, w, n_maps)
        ds.close()
    return dict(workload=EB.WORKLOAD, maps=n_maps, frame=list(SHAPE), metric_keys=keys, **out)


def step_plain(n_maps):
    """Tester.run over a folder of images without ground truth: nothing of the new dataset runs"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cityscapes_eval.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.parent_tree) if a.step.startswith("parent") else ROOT)
        EB.begin_step()
        return EB.end_step(step_metrics(a.reps) if a.step == "metrics" else step_tester(a.maps) if a.step == "tester" else step_plain(a.maps))
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
