#!/usr/bin/env python
"""Pin the scale-and-shift-invariant evaluation to the reference: writes tests/golden/ssi_eval.npz.

BUILD BOX ONLY (needs the reference checkout; leaves oracle/ untouched).  Imports the reference's own estimator/models/losses.py under
oracle.refharness.install(), as tools/make_edge_golden.py imports estimator/utils/metric.py (whose loader is reused here for
compute_metrics).  Stubbed because absent, none of them arithmetic under test: kornia and kornia.losses (dice_loss / focal_loss are
imported, never called), mmengine's print_log and the registry (refharness), estimator.utils.RandomBBoxQueries.

Per case it records the fp32 inputs, the mask, and what the reference computes on the inputs cast to float64 (the yardstick):
compute_scale_and_shift, ScaleAndShiftInvariantLoss with (ssi), (ssi, grad_matching), (grad_matching alone) and (inverse), and
compute_metrics of the aligned prediction (scale * pred + shift rounded once to fp32, widened again; min / max depth as their fp32
values, which is what an fp32 prediction is clamped to).  The same four losses on the fp32
tensors are recorded for information (``*/loss_f32``): the reference reduces in the input's dtype.

Two properties of the reference decide how it is called:
  * forward() squeezes its inputs and then indexes three dimensions, so it fails on a batch of one: every frame is passed twice, the
    value is then the frame's own (2 x sum / 2 x N);
  * it multiplies by the mask where the product never looks outside it, so a NaN outside the mask poisons its sums: the maps it gets
    have every pixel outside the mask set to 0 (``clean``); the recorded inputs keep their holes, NaN and out-of-range values.
The N <= 1 case records no loss: the reference returns ``prediction * 0.0`` there, a training guard; the evaluation reports NaN.

    python tools/make_ssi_golden.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "ssi_eval.npz")
MN, MX = 0.1, 10.0
ERR_KEYS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel")
LOSS_MODES = (dict(ssi=True), dict(ssi=True, grad_matching=True), dict(ssi=False, grad_matching=True), dict(inverse=True))  # l1, gm_ssi, gm, inv


def load_reference():
    import make_edge_golden
    metric = make_edge_golden.load_reference_metric()  # installs refharness, estimator.utils and its own stubs
    ko = sys.modules["kornia"]
    kol = types.ModuleType("kornia.losses")
    kol.dice_loss = kol.focal_loss = None
    ko.losses = kol
    sys.modules["kornia.losses"] = kol
    u = sys.modules["estimator.utils"]
    u.RandomBBoxQueries = object
    for name in ("get_boundaries", "compute_metrics", "compute_boundary_metrics", "extract_edges"):
        setattr(u, name, getattr(metric, name))
    import importlib
    return importlib.import_module("estimator.models.losses"), metric


def garg(h, w):
    return int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w)


def cases():
    """name -> (gt fp32, pred fp32, crop or None).  The prediction's variance is a tenth of its squared mean or more (the conditioning
    of the determinant the GPU test's bound assumes)."""
    rng = np.random.default_rng(20261019)
    out = {}

    def scene(h, w, noise):
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        gt = 4.5 + 3.5 * np.sin(x / (3 + w / 9)) * np.cos(y / (2 + h / 7)) + 0.8 * (x > 0.6 * w)
        pr = 0.8 * gt - 0.4 + noise * rng.standard_normal((h, w)) + 0.6 * (y > 0.5 * h)
        return gt, pr
    for h, w in ((2, 7), (5, 7)):
        gt = rng.uniform(0.5, 9.0, (h, w))
        pr = 0.5 * gt + 0.7 + 0.8 * rng.standard_normal((h, w))
        gt[h - 1, 2] = 0.0
        out[f"t{h}x{w}"] = (gt, pr, None)
    gt, pr = scene(37, 53, 0.25)
    gt[5:9, 10:20] = 0.0          # holes
    gt[20:23, 30:41] = 12.5       # above max_depth
    gt[30, 7] = np.nan            # a NaN is not valid
    gt[rng.random(gt.shape) < 0.1] = 0.0
    pr[6, 12] = np.nan            # (outside the mask: never looked at)
    out["holes37x53"] = (gt, pr, None)
    out["garg37x53"] = (gt, pr, garg(37, 53))
    # 270 x 480: several row blocks whatever their height; values exact in fp16 so that the file stays small
    gt, pr = scene(270, 480, 0.3)
    gt[rng.random(gt.shape) < 0.15] = 0.0
    gt[100:140, 200:260] = 0.0
    gt[8, 8] = np.nan
    out["big270x480"] = (gt.astype(np.float16), pr.astype(np.float16), None)
    # a constant prediction on a power-of-two pixel count: det == 0 exactly -> scale = shift = 0
    out["constpred8x16"] = (rng.uniform(1.0, 9.0, (8, 16)), np.full((8, 16), 2.0), None)
    # N <= 1
    gt = np.zeros((5, 7))
    gt[2, 3] = 3.0
    out["single5x7"] = (gt, rng.uniform(1.0, 9.0, (5, 7)), None)
    return {k: (np.asarray(g).astype(np.float32), np.asarray(p).astype(np.float32), c) for k, (g, p, c) in out.items()}


def mask_of(gt, crop):
    h, w = gt.shape
    y0, y1, x0, x1 = crop or (0, h, 0, w)
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    with np.errstate(invalid="ignore"):
        return m & (gt > np.float32(MN)) & (gt < np.float32(MX))


def main():
    losses, metric = load_reference()
    rec, names = {"min_depth": np.float64(MN), "max_depth": np.float64(MX), "err_keys": np.array(ERR_KEYS)}, []
    for name, (gt, pr, crop) in cases().items():
        names.append(name)
        m = mask_of(gt, crop)
        small = name.startswith("big")
        rec[f"{name}/gt"], rec[f"{name}/pred"] = (gt.astype(np.float16), pr.astype(np.float16)) if small else (gt, pr)
        if small:
            assert np.array_equal(rec[f"{name}/gt"].astype(np.float32), gt, equal_nan=True) and np.array_equal(rec[f"{name}/pred"].astype(np.float32), pr)
        rec[f"{name}/mask"] = np.packbits(m) if small else m
        rec[f"{name}/crop"] = np.array(crop if crop else (0, gt.shape[0], 0, gt.shape[1]), np.int64)
        rec[f"{name}/n"] = np.float64(m.sum())
        if m.sum() <= 1:
            continue
        pm = pr[m].astype(np.float64)
        assert name.startswith("constpred") or pm.var() >= 0.1 * pm.mean() ** 2, (name, pm.var(), pm.mean() ** 2)
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            g = torch.from_numpy(np.where(m, gt, np.float32(0))).to(dt)   # clean: nothing but zeros outside the mask
            p = torch.from_numpy(np.where(m, pr, np.float32(0))).to(dt)
            tm = torch.from_numpy(m)
            two = lambda t: torch.stack([t, t])[:, None]  # noqa: E731
            val = [float(losses.ScaleAndShiftInvariantLoss(**kw)(two(p), two(g), None, two(tm), MN, MX)) for kw in LOSS_MODES]
            rec[f"{name}/loss_{tag}"] = np.array(val, np.float64)
            if tag == "f64":
                s, t = losses.compute_scale_and_shift(p[None], g[None], tm[None])
                rec[f"{name}/scale_shift"] = np.array([float(s[0]), float(t[0])], np.float64)
                aligned = (s[0] * p + t[0]).float().double()  # rounded once to fp32
                # (the bounds as the fp32 values an fp32 prediction is clamped to: float64 arithmetic, the reference's fp32 decisions)
                e = metric.compute_metrics(g, aligned, interpolate=False, garg_crop=False, eigen_crop=False, dataset="",
                                           min_depth_eval=float(np.float32(MN)), max_depth_eval=float(np.float32(MX)))
                rec[f"{name}/errors"] = np.array([float(e[k]) for k in ERR_KEYS], np.float64)
        print(f"  {name}: N {int(m.sum())} scale/shift {rec[f'{name}/scale_shift']} loss {rec[f'{name}/loss_f64']} (fp32 {rec[f'{name}/loss_f32']})")
    rec["cases"] = np.array(names)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
