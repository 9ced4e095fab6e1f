#!/usr/bin/env python
"""U4K dataset evaluation cost: one JSON line (also written to ``--out``, default profiles/u4k_eval_bench.json).

  python tools/bench_u4k_eval.py [--reps 20] [--maps 4] [--skip-tester] [--out PATH]

A synthetic U4K tree at 2160 x 3840 (raw BGR images, disparity .npy, extrinsics, a split file) is written to a temporary directory.

- ``fused_ms``: per frame, ground-truth preparation and scoring on the fused route -- H2D of the disparity from pinned memory,
  ops.disp_gt (depth + boundary in one pass), metrics.compute_metrics_fused (one launch sequence, one D2H) -- plus the image decode
  (H2D of the raw bytes + ops.u8_image) and the three-set scoring (``region``) that replaces the three calls of --edge-metrics.
- ``parent_ms``: the same work on the route that existed before: numpy ``factor / disp`` and metrics.get_boundaries on the host,
  metrics.compute_metrics_device (once, and three times with additional_mask for the three sets), the numpy image expression + H2D.
  Both are wall-clock medians of ``--reps`` calls (parent: of 5) with a device synchronisation at each end, after a warm-up.
- ``tester_maps_s``: Tester.run on v2_zoe_4k_r32 (synthetic weights, f16f6) over UnrealStereo4kDataset, with ground truth (decoded
  and scored) and with the ground truth dropped from the items (nothing scored).
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import evalbench as EB  # noqa: E402
from evalbench import wall_ms  # noqa: E402
RAW = (2160, 3840)
MIN_DEPTH, MAX_DEPTH = 1e-3, 80


def write_tree(root, n, shape=RAW):
    """n frames of scene 00000: Image0/<k>.raw, Disp0/<k>.npy, Extrinsics0|1/<k>.txt, splits/val.txt -> the split path"""
    h, w = shape
    for sub in ("Image0", "Disp0", "Extrinsics0", "Extrinsics1"):
        os.makedirs(os.path.join(root, "00000", sub), exist_ok=True)
    os.makedirs(os.path.join(root, "splits"), exist_ok=True)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    lines = []
    for k in range(n):
        name = f"{k:05d}"
        np.random.default_rng(k).integers(0, 256, (h, w, 3), dtype=np.uint8).tofile(os.path.join(root, "00000", "Image0", name + ".raw"))
        disp = 30.0 + 60.0 * (x > (0.4 + 0.02 * k) * w) + 25.0 * (np.hypot(x - 0.25 * w, y - 0.5 * h) < 0.2 * h) + 2.0 * np.sin(y / 37.0) * np.cos(x / 53.0)
        np.save(os.path.join(root, "00000", "Disp0", name + ".npy"), disp.astype(np.float32))
        for cam, tx in (("Extrinsics0", 0.0), ("Extrinsics1", 0.5)):
            with open(os.path.join(root, "00000", cam, name + ".txt"), "w") as f:
                f.write(f"960.0 0.0 {w / 2} 0.0 960.0 {h / 2} 0.0 0.0 1.0\n1.0 0.0 0.0 {tx} 0.0 1.0 0.0 0.0 0.0 0.0 1.0 0.0\n")
        lines.append(f"00000/Image0/{name}.png 00000/Image1/{name}.png 00000/Disp0/{name}.npy 00000/Disp1/{name}.npy")
    split = os.path.join(root, "splits", "val.txt")
    with open(split, "w") as f:
        f.write("\n".join(lines) + "\n")
    return split


def routes_ms(root, reps):
    from patchrefinerv2_amd import metrics as M, ops
    factor = np.float32(480.0)
    disp = np.load(os.path.join(root, "00000", "Disp0", "00000.npy")).astype(np.float32)
    raw = np.fromfile(os.path.join(root, "00000", "Image0", "00000.raw"), dtype=np.uint8).reshape(*RAW, 3)
    disp_pin, raw_pin = torch.from_numpy(disp).pin_memory(), torch.from_numpy(raw).pin_memory()
    gt_dev = torch.from_numpy(factor / disp).cuda()
    pred = (gt_dev * (1 + 0.05 * torch.sin(torch.arange(RAW[1], device="cuda") / 11.0)))[None, None].contiguous()
    region = M.edge_split_masks_device(gt_dev)
    kw = dict(min_depth_eval=MIN_DEPTH, max_depth_eval=MAX_DEPTH, garg_crop=False, eigen_crop=False, dataset="")
    st = {}

    def fused_prep():
        st["depth"], st["boundary"] = ops.disp_gt(disp_pin.cuda(non_blocking=True), float(factor), 1.0)

    def fused_score():
        return M.compute_metrics_fused(st["depth"], pred, disp_gt_edges=st["boundary"], **kw)

    def fused_score3():
        return M.compute_metrics_fused(st["depth"], pred, disp_gt_edges=st["boundary"], region=region, **kw)

    def parent_prep():
        st["gt_host"] = torch.from_numpy(factor / disp)[None, None]
        st["edges_host"] = torch.from_numpy(M.get_boundaries(disp, th=1, dilation=0))

    def parent_score():
        return M.compute_metrics_device(st["gt_host"], pred, disp_gt_edges=st["edges_host"], **kw)

    def parent_score3():
        return [M.compute_metrics_device(st["gt_host"], pred, disp_gt_edges=st["edges_host"], additional_mask=m, **kw)
                for m in (None, region, ~region)]

    fused = dict(gt_prep=wall_ms(fused_prep, reps), score=wall_ms(fused_score, reps), score_three_sets=wall_ms(fused_score3, reps),
                 image=wall_ms(lambda: ops.u8_image(raw_pin.cuda(non_blocking=True), swap_rb=True), reps))
    parent = dict(gt_prep=wall_ms(parent_prep, 5, warm=1), score=wall_ms(parent_score, 5, warm=1), score_three_sets=wall_ms(parent_score3, 5, warm=1),
                  image=wall_ms(lambda: torch.from_numpy((raw.astype(np.float32)[:, :, ::-1].copy() / 255.0).transpose(2, 0, 1)).cuda(), 5, warm=1))
    for d in (fused, parent):
        d["gt_prep_plus_score"] = round(d["gt_prep"] + d["score"], 3)
    a, b = fused_score(), parent_score()
    agree = max(abs(a[k] - b[k]) / max(1e-12, abs(b[k])) for k in b)
    return fused, parent, agree


def tester_maps_s(root, split, n_maps):
    from patchrefinerv2_amd.tester import UnrealStereo4kDataset
    w, model = EB.workload_model()
    ds = UnrealStereo4kDataset("infer", root, split, dict(network_process_size=[384, 512]), MIN_DEPTH, MAX_DEPTH, image_raw_shape=w["raw"])
    out, _keys = EB.gt_pair_maps_s(model, ds, w, n_maps)
    ds.close()
    return dict(workload=EB.WORKLOAD, maps=n_maps, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--maps", type=int, default=4)
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "u4k_eval_bench.json"))
    a = ap.parse_args()
    EB.begin_step()
    with tempfile.TemporaryDirectory() as root:
        split = write_tree(root, 1 if a.skip_tester else a.maps)
        fused, parent, agree = routes_ms(root, a.reps)
        out = dict(frame=list(RAW), fused_ms=fused, parent_ms=parent, max_rel_diff_fused_vs_parent=float(f"{agree:.3e}"))
        if not a.skip_tester:
            out["tester_maps_s"] = tester_maps_s(root, split, a.maps)
    EB.report(out, a.out)


if __name__ == "__main__":
    main()
