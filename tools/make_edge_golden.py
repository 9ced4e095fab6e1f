#!/usr/bin/env python
"""Pin the host edge metrics to the reference: writes tests/golden/edge_metrics.npz.

BUILD BOX ONLY (needs the reference checkout, REF below; leaves oracle/ untouched).  Imports the reference's own
estimator/utils/metric.py under oracle.refharness.install() -- as oracle/make_golden.py's output-stage generator does -- with two
un-vendored dependencies stubbed:
  skimage.feature.canny          -> patchrefinerv2_amd.metrics.canny (the product's restatement; its parity with skimage is the
                                    part this file cannot pin);
  kornia.filters.gaussian_blur2d -> a direct restatement (normalised exp(-x^2 / 2 sigma^2) taps, separable, reflect border).
The reference's metric_dict needs torchmetrics (absent): the Binary{Precision,Recall,F1Score,HammingDistance,Accuracy} values are
computed from the confusion counts (zero denominator -> 0, torchmetrics' default).
Then runs the reference's extract_edges (preprocess 'log' / 'inv' / 'none') and compute_boundary_metrics on small synthetic maps:
steps, ramps, an empty prediction, no valid GT edges and the EdgeComp quirk (GT edges far from every predicted edge).

    python tools/make_edge_golden.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "edge_metrics.npz")
H, W = 96, 128


def kornia_gaussian_blur2d(x, kernel_size, sigma, border_type="reflect", separable=True):
    """kornia.filters.gaussian_blur2d restated: per-axis taps exp(-(i - k // 2)^2 / (2 sigma^2)) normalised, reflect padding,
    separable correlation (rows then columns)"""
    x = torch.as_tensor(x).float()
    ky, kx = kernel_size
    sy, sx = sigma

    def taps(k, s):
        i = torch.arange(k, dtype=torch.float32) - k // 2
        g = torch.exp(-(i ** 2) / (2.0 * float(s) ** 2))
        return g / g.sum()
    c = x.shape[1]
    x = F.pad(x, (kx // 2, kx // 2, ky // 2, ky // 2), mode=border_type)
    x = F.conv2d(x, taps(kx, sx).view(1, 1, 1, kx).repeat(c, 1, 1, 1), groups=c)
    return F.conv2d(x, taps(ky, sy).view(1, 1, ky, 1).repeat(c, 1, 1, 1), groups=c)


def load_reference_metric():
    from oracle import refharness
    from patchrefinerv2_amd import metrics as M
    refharness.install()
    sk, skf = types.ModuleType("skimage"), types.ModuleType("skimage.feature")
    skf.canny = lambda image, sigma=1.0, mask=None: M.canny(image, sigma=sigma)
    sk.feature = skf
    ko, kof = types.ModuleType("kornia"), types.ModuleType("kornia.filters")
    kof.gaussian_blur2d = kornia_gaussian_blur2d
    ko.filters = kof
    sys.modules.update({"skimage": sk, "skimage.feature": skf, "kornia": ko, "kornia.filters": kof})
    for name in ("imageio",):
        sys.modules.setdefault(name, types.ModuleType(name))
    u = types.ModuleType("estimator.utils")
    u.__path__ = [os.path.join(refharness.REF, "estimator/utils")]
    sys.modules["estimator.utils"] = u
    import importlib
    return importlib.import_module("estimator.utils.metric")


def metric_dict():
    from patchrefinerv2_amd.metrics import binary_scores

    def scorer(key):
        def f(pred_flat, gt_flat):
            p, g = pred_flat.bool(), gt_flat.bool()
            tp, fp, fn = int((p & g).sum()), int((p & ~g).sum()), int((~p & g).sum())
            return binary_scores(tp, fp, fn, int(p.numel()) - tp - fp - fn)[key]
        return f
    return {k: scorer(k) for k in ("precision", "recall", "f1_score", "hamming", "acc")}


def cases():
    rng = np.random.default_rng(1234)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    smooth = lambda s: 0.05 * np.sin(x / (7 + s)) * np.cos(y / (11 + s))  # noqa: E731
    out = {}
    # steps: two depth planes and a box, the prediction's discontinuities moved by a pixel or two
    gt = 2.0 + 3.0 * (x > 0.45 * W) + 1.5 * ((abs(y - 48) < 20) & (abs(x - 30) < 18)) + smooth(0)
    pr = 2.0 + 3.0 * (x > 0.45 * W + 2) + 1.5 * ((abs(y - 49) < 20) & (abs(x - 31) < 18)) + smooth(1)
    out["steps"] = (gt, pr, (gt > 0.1) & (gt < 10))
    # ramps: an oblique ramp with a diagonal step; the prediction is noisy
    gt = 1.0 + 0.03 * x + 0.02 * y + 2.5 * (x + 0.7 * y > 110)
    pr = gt * (1 + 0.01 * rng.standard_normal(gt.shape)) + 0.3 * (x - 0.5 * y > 60)
    valid = (gt > 0.1) & (gt < 10)
    valid[:6] = False
    out["ramps"] = (gt, pr, valid)
    # empty prediction: a constant map has no edges (EdgeAcc = EdgeComp = th)
    gt = 3.0 + 2.0 * (y > 40) + smooth(2)
    out["empty_pred"] = (gt, np.full_like(gt, 4.0), (gt > 0.1) & (gt < 10))
    # no valid GT edges: the only discontinuity lies outside the valid region
    gt = 3.0 + 2.0 * (x > 100)
    pr = 3.0 + 2.0 * (x > 98) + 1.0 * (y > 50)
    out["no_valid_gt_edges"] = (gt, pr, x < 80)
    # EdgeComp quirk: GT edges far (> th_edges_comp) from every predicted edge still enter EdgeComp's mean
    gt = 2.0 + 3.0 * (x > 30) + 2.0 * (y > 70) + 1.0 * (x > 110)
    pr = 2.0 + 3.0 * (x > 31)
    out["edgecomp_quirk"] = (gt, pr, np.ones_like(gt, bool))
    # depth <= 0 / holes: the 'none' preprocessing sends them to -inf
    gt = 2.0 + 3.0 * (x > 64) + smooth(3)
    gt[30:40, 20:30] = 0.0
    out["holes"] = (gt, gt * 1.02, (gt > 0.1) & (gt < 10))
    return {k: (g.astype(np.float32), p.astype(np.float32), v.astype(bool)) for k, (g, p, v) in out.items()}


def main():
    metric = load_reference_metric()
    md = metric_dict()
    keys = ("EdgeAcc", "EdgeComp", "precision", "recall", "f1_score", "hamming", "acc")
    rec = {"metric_keys": np.array(keys)}
    names = []
    for name, (gt, pr, valid) in cases().items():
        names.append(name)
        rec[f"{name}/gt"], rec[f"{name}/pred"], rec[f"{name}/valid"] = gt, pr, valid
        for mode in ("log", "inv", "none"):
            rec[f"{name}/gt_edges_{mode}"] = np.asarray(metric.extract_edges(gt.copy(), preprocess=mode), bool)
        pe = np.asarray(metric.extract_edges(pr.copy(), preprocess="log"), bool)
        rec[f"{name}/pred_edges_log"] = pe
        ge = rec[f"{name}/gt_edges_log"]
        m = metric.compute_boundary_metrics(torch.from_numpy(gt), torch.from_numpy(pr), gt_edges=torch.from_numpy(ge.copy()),
                                            valid_mask=torch.from_numpy(valid.copy()), pred_edges=torch.from_numpy(pe.copy()), metric_dict=md)
        rec[f"{name}/metrics"] = np.array([float(m[k]) for k in keys], np.float64)
        print(f"  {name}: gt edges {int(ge.sum())}, pred edges {int(pe.sum())},", {k: round(float(m[k]), 6) for k in keys})
    rec["cases"] = np.array(names)
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
