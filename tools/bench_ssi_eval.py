#!/usr/bin/env python
"""Cost of the scale-and-shift-invariant evaluation (metrics.compute_ssi_metrics_fused, csrc/ssi_eval.hip): one JSON line (also written
to ``--out``, default profiles/ssi_eval.json).

  python tools/bench_ssi_eval.py [--reps 20] [--maps 3] [--skip-tester] [--parent-tree DIR] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- step ``fixture``: the op on every scored case of tests/golden/ssi_eval.npz -> the largest relative deviation of any key from the
  reference's recorded float64 result (the figure tests/test_ssi_eval_gpu.py bounds by 1e-9).
- steps ``4k`` (2160 x 3840), ``eth3d`` (ground truth 4032 x 6048, prediction 2160 x 3840, the resize inside the kernels) and
  ``cityscapes`` (1024 x 2048), per frame:
    ``new_ms``     metrics.compute_ssi_metrics_fused: two fused passes, the fits solved on the device, one D2H;
    ``torch_ms``   the same quantities written with torch ops on the device, as a user would on the parent commit: F.interpolate first,
                   the reference's formulas (losses.py:523-544, :600-700) in float64, metrics.compute_metrics_device on the aligned map.
  Wall-clock medians of ``--reps`` calls (torch: of 3) with a device synchronisation at each end, after a warm-up; ``*_alloc_bytes``:
  device bytes ALLOCATED per frame, from the caching allocator's counter (``allocated_bytes.all.allocated``) around one call.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over a synthetic ETH3D-format ground-truth folder with
  ``ssi_metrics`` off and on.  ``--parent-tree DIR`` (a built checkout of the parent commit): the same run, flag off, with that tree's
  package, as ``parent``.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from evalbench import alloc_bytes, wall_ms  # noqa: E402

MIN_DEPTH, MAX_DEPTH = 1e-3, 80
SIZES = {"4k": ((2160, 3840), (2160, 3840)), "eth3d": ((4032, 6048), (2160, 3840)), "cityscapes": ((1024, 2048), (1024, 2048))}  # (gt, pred)
STEPS = ("fixture", "4k", "eth3d", "cityscapes", "tester", "parent")


def depth_map(shape, k=0):
    """metric depth with planes, a disc, fine texture and holes (0 / NaN), float32"""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    d = 3.0 + 6.0 * (x > (0.55 + 0.02 * k) * w) + 2.5 * (np.hypot(x - 0.25 * w, y - 0.5 * h) < 0.18 * h) + 0.2 * np.sin(y / 37.0) * np.cos(x / 53.0)
    d = d.astype(np.float32)
    d[::97, ::89] = 0.0
    d[5::211, 7::193] = np.nan
    return d


def ssi_torch(gt, pred, mn, mx):
    """the fifteen keys with torch ops on the device: losses.py's formulas in float64 on the resized prediction"""
    from patchrefinerv2_amd import metrics as M
    if pred.shape[-2:] != gt.shape[-2:]:
        pred = F.interpolate(pred, gt.shape[-2:], mode="bilinear", align_corners=False)
    g32, p32 = gt.reshape(gt.shape[-2:]), pred.reshape(pred.shape[-2:])
    m = (g32 > mn) & (g32 < mx)
    zero = torch.zeros((), dtype=torch.float64, device=gt.device)
    g, p = torch.where(m, g32.double(), zero), torch.where(m, p32.double(), zero)

    def fit(p, g, m):  # compute_scale_and_shift
        md = m.double()
        a00, a01, a11, b0, b1 = (md * p * p).sum(), (md * p).sum(), md.sum(), (md * p * g).sum(), (md * g).sum()
        det = a00 * a11 - a01 * a01
        if not bool(det > 0):
            return zero, zero
        return (a11 * b0 - a01 * b1) / det, (-a01 * b0 + a00 * b1) / det

    def gm(d, vm, hm):
        return ((d[:-2] - d[2:]).abs() * vm).sum() + ((d[:, :-2] - d[:, 2:]).abs() * hm).sum()
    n = m.sum()
    vm, hm = m[:-2] & m[2:], m[:, :-2] & m[:, 2:]
    s, t = fit(p, g, m)
    vp, vg, hp, hg = p[:-2] - p[2:], g[:-2] - g[2:], p[:, :-2] - p[:, 2:], g[:, :-2] - g[:, 2:]
    sv, tv = fit(vp, vg, vm)
    sh, th = fit(hp, hg, hm)
    md = m.double()
    out = dict(ssi_scale=s, ssi_shift=t, ssi_l1=((s * p + t - g).abs() * md).sum() / n, ssi_gm=gm((s * p + t - g) * md, vm, hm) / n,
               gm=gm((p - g) * md, vm, hm) / n,
               ssi_gm_inv=(((sv * vp + tv - vg).abs() * vm).sum() + ((sh * hp + th - hg).abs() * hm).sum()) / n)
    out = {k: float(v) for k, v in out.items()}
    aligned = (out["ssi_scale"] * p32.double() + out["ssi_shift"]).float()
    errs = M.compute_metrics_device(gt, aligned[None, None], garg_crop=False, eigen_crop=False, dataset="", min_depth_eval=mn, max_depth_eval=mx)
    out.update({"ssi_" + k: float(v) for k, v in errs.items()})
    return out


def step_fixture():
    from patchrefinerv2_amd import metrics as M, ops
    z = np.load(os.path.join(ROOT, "tests", "golden", "ssi_eval.npz"))
    mn, mx, worst = float(z["min_depth"]), float(z["max_depth"]), {}
    for name in (str(n) for n in z["cases"]):
        if float(z[f"{name}/n"]) <= 1:
            continue
        gt, pred = (torch.from_numpy(z[f"{name}/{k}"].astype(np.float32)).cuda()[None] for k in ("gt", "pred"))
        got = M.ssi_from_values(ops.ssi_metrics(gt, pred, mn, mx, tuple(int(v) for v in z[f"{name}/crop"]))[0].cpu().numpy())
        want = list(z[f"{name}/scale_shift"]) + list(z[f"{name}/loss_f64"]) + list(z[f"{name}/errors"])
        worst[name] = max(abs(got[k] - w) / abs(w) if w else abs(got[k]) for k, w in zip(M.SSI_KEYS, want))
    return dict(bound=1e-9, max_rel_deviation=float(f"{max(worst.values()):.3e}"), per_case={k: float(f"{v:.3e}") for k, v in worst.items()})


def step_size(step, reps):
    from patchrefinerv2_amd import metrics as M
    gt_shape, pred_shape = SIZES[step]
    gt = torch.nan_to_num(torch.from_numpy(depth_map(gt_shape)).cuda(), nan=0.0)[None, None]
    lo = F.interpolate(gt, pred_shape, mode="bilinear", align_corners=False) if pred_shape != gt_shape else gt
    xx = torch.arange(pred_shape[1], device="cuda")
    pred = (0.6 * lo.clamp(min=0.5) * (1 + 0.05 * torch.sin(xx / 11.0)) + 0.8).contiguous()
    kw = dict(garg_crop=False, eigen_crop=False, dataset="", min_depth_eval=MIN_DEPTH, max_depth_eval=MAX_DEPTH)

    def new():
        return M.compute_ssi_metrics_fused(gt, pred, fuse_resize=True, **kw)

    def parent():
        return ssi_torch(gt, pred, MIN_DEPTH, MAX_DEPTH)
    a, b = new(), parent()
    agree = max(abs(a[k] - b[k]) / max(1e-12, abs(b[k])) for k in b)
    moved = 4.0 * 2 * (gt_shape[0] * gt_shape[1] + pred_shape[0] * pred_shape[1])  # two passes over the two maps
    new_ms = wall_ms(new, reps)
    return dict(gt=list(gt_shape), pred=list(pred_shape), new_ms=new_ms, torch_ms=wall_ms(parent, 3, warm=1),
                new_alloc_bytes=alloc_bytes(new), torch_alloc_bytes=alloc_bytes(parent), map_bytes_two_passes=int(moved),
                new_gb_per_s=round(moved / new_ms / 1e6, 1), max_rel_diff_new_vs_torch=float(f"{agree:.3e}"))


def step_tester(n_maps, flags):
    from patchrefinerv2_amd.tester import ImageDataset
    gt_shape = SIZES["eth3d"][0]
    w, model = EB.workload_model()
    with tempfile.TemporaryDirectory() as root:
        img_dir, gt_dir = os.path.join(root, "images"), os.path.join(root, "gt")
        os.makedirs(img_dir), os.makedirs(gt_dir)
        for k in range(n_maps):
            np.save(os.path.join(img_dir, f"{k:05d}.npy"), np.random.default_rng(k).integers(0, 256, tuple(w["raw"]) + (3,), dtype=np.uint8))
            depth_map(gt_shape, k).tofile(os.path.join(gt_dir, f"{k:05d}.raw"))
        out = {}
        for tag, extra in flags:
            ds = ImageDataset(img_dir, gt_dir=gt_dir, gt_format="eth3d", gt_shape=gt_shape, image_resolution=w["raw"], min_depth=MIN_DEPTH,
                              max_depth=MAX_DEPTH, **extra)
            out[tag], res, _ = EB.timed_maps_s(model, ds, w, n_maps)
            out[tag + "_keys"] = len(res[0]["metrics"])
            ds.close()
    return dict(workload=EB.WORKLOAD, maps=n_maps, gt=list(gt_shape), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--maps", type=int, default=3)
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: Tester.run from its package, as 'parent'")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssi_eval.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.parent_tree) if a.step == "parent" else ROOT)
        EB.begin_step()
        if a.step == "fixture":
            res = step_fixture()
        elif a.step == "tester":
            res = step_tester(a.maps, (("ssi_off", {}), ("ssi_on", dict(ssi_metrics=True))))
        elif a.step == "parent":
            res = step_tester(a.maps, (("ssi_off", {}),))
        else:
            res = step_size(a.step, a.reps)
        return EB.end_step(res)
    steps = [s for s in STEPS if not (a.skip_tester and s in ("tester", "parent")) and not (s == "parent" and not a.parent_tree)]
    out = EB.run_steps(__file__, steps, a.step_timeout,
                       ["--reps", a.reps, "--maps", a.maps] + (["--parent-tree", a.parent_tree] if a.parent_tree else []))
    if "tester" in out:
        t = out["tester"]
        t["ssi_overhead_pct"] = round(100 * (t["ssi_off"] / t["ssi_on"] - 1), 2)
    return EB.report(out, a.out)


if __name__ == "__main__":
    sys.exit(main())
