#!/usr/bin/env python
"""Cost of the scale-invariant boundary F1 (metrics.compute_boundary_f1_fused, csrc/boundary_eval.hip): one JSON line (also written to
``--out``, default profiles/boundary_f1.json).

  python tools/bench_boundary_f1.py [--reps 20] [--maps 3] [--skip-tester] [--parent-tree DIR] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- steps ``4k`` (2160 x 3840), ``eth3d`` (ground truth 4032 x 6048, prediction 2160 x 3840, the resize inside the kernel) and
  ``cityscapes`` (1024 x 2048), per frame:
    ``new_ms``     metrics.compute_boundary_f1_fused: one fused pass of integer counts, one D2H;
    ``torch_ms``   the same definition written with torch boolean ops on the device: F.interpolate first, then per ratio and direction
                   the flag maps of prediction and ground truth and their sums.
  Wall-clock medians of ``--reps`` calls (torch: of 3) with a device synchronisation at each end, after a warm-up; ``*_alloc_bytes``:
  device bytes ALLOCATED per frame, from the caching allocator's counter (``allocated_bytes.all.allocated``) around one call;
  ``counts_equal``: whether the two routes give the same 122 counts.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over a synthetic ETH3D-format ground-truth folder with
  ``boundary_f1`` off and on.  ``--parent-tree DIR`` (a built checkout of the parent commit): three alternating runs of the unchanged
  path (flag off), this tree's package against that tree's, as ``unchanged``; the path counts as unchanged when the two sets of
  three lie inside each other's spread, that is their ranges overlap (``inside_each_others_spread``).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from bench_ssi_eval import MAX_DEPTH, MIN_DEPTH, SIZES, depth_map, step_tester  # noqa: E402
from evalbench import alloc_bytes, wall_ms  # noqa: E402

ALTERNATIONS = 3
STEPS = ("4k", "eth3d", "cityscapes", "tester") + tuple(f"{side}{k}" for k in range(ALTERNATIONS) for side in ("this", "parent"))


def boundary_torch(gt, pred, mn, mx, thresholds):
    """the row of ops.boundary_f1 with torch boolean ops on the device: every flag map is materialised"""
    if pred.shape[-2:] != gt.shape[-2:]:
        pred = F.interpolate(pred, gt.shape[-2:], mode="bilinear", align_corners=False)
    g, p = gt.reshape(gt.shape[-2:]), pred.reshape(pred.shape[-2:])
    m = (g > mn) & (g < mx)
    p = torch.where(torch.isnan(p), torch.full_like(p, mn), p).clamp(mn, mx)
    one = torch.ones((), dtype=g.dtype, device=g.device)
    g, p = torch.where(m, g, one), torch.where(m, p, one)
    hm, vm = m[:, :-1] & m[:, 1:], m[:-1] & m[1:]

    def flags(d, t):
        ha, hb, va, vb = d[:, :-1], d[:, 1:], d[:-1], d[1:]
        return (ha > t * hb) & hm, (va > t * vb) & vm, (hb > t * ha) & hm, (vb > t * va) & vm
    row = [hm.sum(), vm.sum()]
    for t in thresholds:
        t = float(t)
        for fp, fg in zip(flags(p, t), flags(g, t)):
            row += [(fp & fg).sum(), fp.sum(), fg.sum()]
    return torch.stack(row).double().cpu().numpy()  # one D2H


def step_size(step, reps):
    from patchrefinerv2_amd import metrics as M, ops
    gt_shape, pred_shape = SIZES[step]
    gt = torch.nan_to_num(torch.from_numpy(depth_map(gt_shape)).cuda(), nan=0.0)[None, None]
    lo = F.interpolate(gt, pred_shape, mode="bilinear", align_corners=False) if pred_shape != gt_shape else gt
    xx = torch.arange(pred_shape[1], device="cuda")
    pred = (0.6 * lo.clamp(min=0.5) * (1 + 0.05 * torch.sin(xx / 11.0)) + 0.8).contiguous()
    kw = dict(garg_crop=False, eigen_crop=False, dataset="", min_depth_eval=MIN_DEPTH, max_depth_eval=MAX_DEPTH)
    th = M.boundary_thresholds()

    def new():
        return M.compute_boundary_f1_fused(gt, pred, fuse_resize=True, **kw)

    def parent():
        return M.boundary_from_values(boundary_torch(gt, pred, MIN_DEPTH, MAX_DEPTH, th), th)
    row = ops.boundary_f1(gt[0], pred[0], MIN_DEPTH, MAX_DEPTH, None, th)[0].cpu().numpy()
    want = boundary_torch(gt, pred, MIN_DEPTH, MAX_DEPTH, th)
    moved = 4.0 * (gt_shape[0] * gt_shape[1] + pred_shape[0] * pred_shape[1])  # one pass over the two maps
    new_ms = wall_ms(new, reps)
    return dict(gt=list(gt_shape), pred=list(pred_shape), new_ms=new_ms, torch_ms=wall_ms(parent, 3, warm=1),
                new_alloc_bytes=alloc_bytes(new), torch_alloc_bytes=alloc_bytes(parent), map_bytes_one_pass=int(moved),
                new_gb_per_s=round(moved / new_ms / 1e6, 1), counts_equal=bool((row == want).all()), pairs=[float(row[0]), float(row[1])],
                gt_boundaries_at_first_ratio=float(row[2:14].reshape(4, 3)[:, 2].sum()), scores=new())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--maps", type=int, default=3)
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: Tester.run from its package, alternating "
                    "with this tree's, flag off")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_f1.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.parent_tree) if a.step.startswith("parent") else ROOT)
        EB.begin_step()
        if a.step == "tester":
            res = step_tester(a.maps, (("boundary_off", {}), ("boundary_on", dict(boundary_f1=True))))
        elif a.step.startswith(("this", "parent")):
            res = step_tester(a.maps, (("boundary_off", {}),))
        else:
            res = step_size(a.step, a.reps)
        return EB.end_step(res)
    steps = [s for s in STEPS if (s in SIZES or not a.skip_tester) and (s in SIZES or s == "tester" or a.parent_tree)]
    out = EB.run_steps(__file__, steps, a.step_timeout,
                       ["--reps", a.reps, "--maps", a.maps] + (["--parent-tree", a.parent_tree] if a.parent_tree else []))
    if "tester" in out:
        t = out["tester"]
        t["boundary_overhead_pct"] = round(100 * (t["boundary_off"] / t["boundary_on"] - 1), 2)
    runs = {side: [out.pop(f"{side}{k}")["boundary_off"] for k in range(ALTERNATIONS) if f"{side}{k}" in out] for side in ("this", "parent")}
    if runs["parent"]:
        (lo_t, hi_t), (lo_p, hi_p) = ((min(v), max(v)) for v in (runs["this"], runs["parent"]))
        out["unchanged"] = dict(workload=EB.WORKLOAD, maps=a.maps, this_maps_s=runs["this"], parent_maps_s=runs["parent"],
                                inside_each_others_spread=bool(lo_t <= hi_p and lo_p <= hi_t))
    return EB.report(out, a.out)


if __name__ == "__main__":
    sys.exit(main())
