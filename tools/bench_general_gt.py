#!/usr/bin/env python
"""Cost of the general dataset's ground truth: one JSON line (also written to ``--out``, default profiles/general_gt_eval.json).

  python tools/bench_general_gt.py [--reps 20] [--maps 4] [--skip-tester] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- step ``eth3d``: ground truth 4032 x 6048 (raw float32), prediction 2160 x 3840; step ``cityscapes``: 1024 x 2048 (uint16 PNG
  samples), prediction 512 x 1024.  Per frame, decode plus scoring on two routes, in one process:
    ``new_ms``     H2D of the raw samples from pinned memory, ops.gt_decode (depth + boundary, one pass) and
                   metrics.compute_metrics_fused(fuse_resize=True): the prediction is sampled inside the scoring kernel;
    ``parent_ms``  the route before this tool existed: the reference's numpy decode and metrics.get_boundaries on the host, then
                   metrics.compute_metrics_fused, which writes F.interpolate(pred -> the ground truth's shape) first.
  Wall-clock medians of ``--reps`` calls (parent: of 3) with a device synchronisation at each end, after a warm-up.
  ``*_alloc_bytes``: device bytes ALLOCATED per frame on each route, read from the caching allocator's counter
  (``allocated_bytes.all.allocated``) around one call; ``resize_bytes_removed`` is the difference between the two scoring calls.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over a synthetic ETH3D-format folder
  (ImageDataset(gt_format='eth3d'), ground truth 4032 x 6048), with ground truth and with it dropped from the items.
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
from evalbench import alloc_bytes, wall_ms  # noqa: E402
MIN_DEPTH, MAX_DEPTH = 1e-3, 80
SIZES = dict(eth3d=((4032, 6048), (2160, 3840)), cityscapes=((1024, 2048), (512, 1024)))
STEPS = ("eth3d", "cityscapes", "tester")


def eth3d_map(shape, k=0):
    """metric depth with planes, a disc, fine texture and holes (inf / NaN), float32"""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    d = 3.0 + 6.0 * (x > (0.4 + 0.02 * k) * w) + 2.5 * (np.hypot(x - 0.25 * w, y - 0.5 * h) < 0.2 * h) + 0.2 * np.sin(y / 37.0) * np.cos(x / 53.0)
    d = d.astype(np.float32)
    d[::97, ::89] = np.inf
    d[5::211, 7::193] = np.nan
    return d


def cityscapes_map(shape):
    h, w = shape
    y, x = np.mgrid[0:h, 0:w]
    v = (3000 + 5000 * (x > 0.45 * w) + 2500 * (np.hypot(x - 0.25 * w, y - 0.5 * h) < 0.2 * h) + (x * 7 + y * 3) % 50).astype(np.uint16)
    v[::97, ::89] = 0
    return v


def step_routes(kind, reps):
    from patchrefinerv2_amd import metrics as M, ops
    gt_shape, pred_shape = SIZES[kind]
    raw = eth3d_map(gt_shape) if kind == "eth3d" else cityscapes_map(gt_shape)
    pin = torch.from_numpy(raw).pin_memory()
    kw = dict(min_depth_eval=MIN_DEPTH, max_depth_eval=MAX_DEPTH, garg_crop=False, eigen_crop=False, dataset="")

    def host_decode():  # the decode rules of general_dataset.py:106-111 / :142-151 in numpy, as a host-side dataset would run them
        with np.errstate(divide="ignore", invalid="ignore"):
            if kind == "eth3d":
                depth = np.where(np.isfinite(raw), raw, np.float32(0))
            else:
                f = raw.astype(np.float32)
                q = np.float32(ops.CITYSCAPES_FACTOR) / np.where(raw > 0, (f - np.float32(1)) / np.float32(256), f)
                depth = np.where(np.isfinite(q), q, np.float32(0))
            depth = np.ascontiguousarray(depth, np.float32)
            return depth, M.get_boundaries(depth, th=1, dilation=0)
    depth_host, edges_host = host_decode()
    gt_dev = torch.from_numpy(depth_host).cuda()
    lo = torch.nn.functional.interpolate(gt_dev[None, None], pred_shape, mode="bilinear", align_corners=False)
    pred = (lo.clamp(min=0.5) * (1 + 0.05 * torch.sin(torch.arange(pred_shape[1], device="cuda") / 11.0))).contiguous()
    st = dict(gt_host=torch.from_numpy(depth_host)[None, None], edges_host=torch.from_numpy(edges_host))

    def new_decode():
        st["depth"], st["boundary"] = ops.gt_decode(pin.cuda(non_blocking=True), kind, th=1.0)

    def new_score():
        return M.compute_metrics_fused(st["depth"], pred, disp_gt_edges=st["boundary"], fuse_resize=True, **kw)

    def two_step_score():  # the same device ground truth, the resize written first: isolates what fuse_resize removes
        return M.compute_metrics_fused(st["depth"], pred, disp_gt_edges=st["boundary"], **kw)

    def parent_decode():
        d, e = host_decode()
        st["gt_host"], st["edges_host"] = torch.from_numpy(d)[None, None], torch.from_numpy(e)

    def parent_score():
        return M.compute_metrics_fused(st["gt_host"], pred, disp_gt_edges=st["edges_host"], **kw)

    new = dict(decode=wall_ms(new_decode, reps), score=wall_ms(new_score, reps))
    two = wall_ms(two_step_score, reps)
    parent = dict(decode=wall_ms(parent_decode, 3, warm=1), score=wall_ms(parent_score, 3, warm=1))
    for d in (new, parent):
        d["decode_plus_score"] = round(d["decode"] + d["score"], 3)
    a, b = new_score(), parent_score()
    agree = max(abs(a[k] - b[k]) / max(1e-12, abs(b[k])) for k in b)
    na, ta = alloc_bytes(new_score), alloc_bytes(two_step_score)
    return dict(gt=list(gt_shape), pred=list(pred_shape), new_ms=new, parent_ms=parent, score_resize_first_ms=two,
                new_alloc_bytes=dict(decode=alloc_bytes(new_decode), score=na), parent_alloc_bytes=dict(decode=0, score=alloc_bytes(parent_score)),
                resize_bytes_removed=ta - na, resized_map_bytes=gt_shape[0] * gt_shape[1] * 4,
                max_rel_diff_new_vs_parent=float(f"{agree:.3e}"))


def step_tester(n_maps):
    from patchrefinerv2_amd.tester import ImageDataset
    gt_shape = SIZES["eth3d"][0]
    w, model = EB.workload_model()
    with tempfile.TemporaryDirectory() as root:
        img_dir, gt_dir = os.path.join(root, "images"), os.path.join(root, "gt")
        os.makedirs(img_dir), os.makedirs(gt_dir)
        for k in range(n_maps):
            np.save(os.path.join(img_dir, f"{k:05d}.npy"), np.random.default_rng(k).integers(0, 256, tuple(w["raw"]) + (3,), dtype=np.uint8))
            eth3d_map(gt_shape, k).tofile(os.path.join(gt_dir, f"{k:05d}.raw"))
        ds = ImageDataset(img_dir, gt_dir=gt_dir, gt_format="eth3d", gt_shape=gt_shape, image_resolution=w["raw"], min_depth=MIN_DEPTH,
                          max_depth=MAX_DEPTH)
        out, _keys = EB.gt_pair_maps_s(model, ds, w, n_maps)
        ds.close()
    return dict(workload=EB.WORKLOAD, maps=n_maps, gt=list(gt_shape), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--maps", type=int, default=4)
    ap.add_argument("--skip-tester", action="store_true")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "general_gt_eval.json"))
    a = ap.parse_args()
    if a.step:
        EB.begin_step()
        return EB.end_step(step_tester(a.maps) if a.step == "tester" else step_routes(a.step, a.reps))
    out = EB.run_steps(__file__, STEPS[:2] if a.skip_tester else STEPS, a.step_timeout, ["--reps", a.reps, "--maps", a.maps])
    return EB.report(out, a.out)


if __name__ == "__main__":
    sys.exit(main())
