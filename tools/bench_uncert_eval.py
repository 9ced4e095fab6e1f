#!/usr/bin/env python
"""Cost of the sparsification scores (metrics.compute_uncertainty_metrics_fused, csrc/sparsify.hip): one JSON line (also written to
``--out``, default profiles/uncert_eval.json).

  python tools/bench_uncert_eval.py [--reps 20] [--maps 3] [--skip-tester] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- step ``deviation``: the fused route against the host specification metrics.compute_uncertainty_metrics on continuous, quantised
  (four values) and count-gated uncertainties at 270 x 480 and 1024 x 2048 -> the largest relative deviation of any curve value (a score
  relative to the largest value of its sparsification curve), and whether every threshold and kept count is equal.
- steps ``4k`` (2160 x 3840) and ``cityscapes`` (1024 x 2048), L = 20, with a count map, per frame:
    ``new_ms``     metrics.compute_uncertainty_metrics_fused: the terms pass, 9 radix selections, the bucket pass, one D2H;
    ``torch_ms``   the same definition written with torch ops on the device (torch.sort of the three key sets, float64 cumulative sums,
                   searchsorted for the ties) -- a baseline to report, not a bar.
  Wall-clock medians of ``--reps`` calls (torch: of 5) with a device synchronisation at each end, after a warm-up; ``*_alloc_bytes``:
  device bytes ALLOCATED per frame, from the caching allocator's counter (``allocated_bytes.all.allocated``) around one call;
  ``workspace_bytes``: prv2_sparsify_workspace_bytes (the three materialised key maps and the mask are 13 bytes per pixel of it).
- ``tests``: the deviation tests/test_uncert_eval_gpu.py measured on its own cases (its MEASURED constant) and the bound it asserts.
- step ``tester``: Tester.generate_pl maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over a small synthetic U4K tree, without and with
  ``uncert_metrics``.
"""
from __future__ import annotations

import argparse
import os
import re
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from evalbench import alloc_bytes, wall_ms  # noqa: E402

MIN_DEPTH, MAX_DEPTH, LEVELS = 1e-3, 80, 20
SIZES = {"4k": (2160, 3840), "cityscapes": (1024, 2048)}
STEPS = ("deviation", "4k", "cityscapes", "tester")


def maps(shape, seed=0, kind="continuous"):
    """gt with holes, a prediction off by a smooth factor and noise, an uncertainty that follows the error loosely, tile counts: fp32"""
    h, w = shape
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    gt = (3.0 + 6.0 * (x > 0.55 * w) + 2.5 * (np.hypot(x - 0.25 * w, y - 0.5 * h) < 0.18 * h) + 0.2 * np.sin(y / 37.0) * np.cos(x / 53.0)).astype(np.float32)
    gt[::97, ::89] = 0.0
    noise = rs.standard_normal((h, w)).astype(np.float32)
    pred = (gt * (1.0 + 0.05 * np.sin(x / 11.0)) + 0.3 * noise).astype(np.float32)
    uncert = (np.abs(0.3 * noise) * (0.5 + rs.random_sample((h, w)).astype(np.float32)) + 0.02 * np.abs(np.sin(x / 11.0))).astype(np.float32)
    if kind == "quantised":
        uncert = (np.floor(uncert * 4 / float(uncert.max())).clip(0, 3) / 4).astype(np.float32)
    count = (1.0 + np.floor(8.0 * np.abs(np.sin(x / 200.0) * np.cos(y / 150.0)))).astype(np.float32)
    return gt, pred, uncert, count


def uncert_torch(gt, pred, uncert, count, min_count, mn, mx, levels):
    """the four scores with torch ops on the device: three torch.sort calls, float64 cumulative sums (finite keys or +inf, no NaN)"""
    valid = (gt > mn) & (gt < mx)
    p = torch.nan_to_num(pred, nan=mn).clamp(mn, mx)
    key = torch.where(count.double() < min_count, torch.full_like(uncert, float("inf")), uncert)
    g, p, key = gt[valid], p[valid], key[valid]
    d = g - p
    e_rel, e_sq = d.abs() / g, d * d
    n = g.numel()
    nk = n - (n * torch.arange(levels, device=gt.device)) // levels

    def curves(K, terms):
        srt, idx = torch.sort(K)
        m = torch.searchsorted(srt, srt[nk - 1].contiguous(), right=True)  # the ties of the threshold are kept
        return [torch.cumsum(t[idx].double(), 0)[m - 1] / m for t in terms]
    s_rel, s_sq = curves(key, (e_rel, e_sq))
    o_rel, = curves(e_rel, (e_rel,))
    o_sq, = curves(e_sq, (e_sq,))
    s_rmse, o_rmse = s_sq.sqrt(), o_sq.sqrt()
    vals = torch.stack([(s_rel - o_rel).mean(), (s_rel[0] - s_rel).mean(), (s_rmse - o_rmse).mean(), (s_rmse[0] - s_rmse).mean()]).cpu()
    return dict(zip(("ause_abs_rel", "aurg_abs_rel", "ause_rmse", "aurg_rmse"), (float(v) for v in vals)))


def rel_deviation(got, want):
    """the largest relative deviation: curve values relative to themselves, scores relative to the largest value of their curve"""
    from patchrefinerv2_amd import metrics as M
    worst = 0.0
    for k in M.UNCERT_CURVES:
        worst = max(worst, float(np.max(np.abs(got[k] - want[k]) / np.abs(want[k]))))
    for k in M.UNCERT_KEYS:
        worst = max(worst, abs(got[k] - want[k]) / float(np.max(np.abs(want["spars_" + k.split("_", 1)[1]]))))
    return worst


def step_deviation():
    from patchrefinerv2_amd import metrics as M
    worst, exact = {}, True
    for shape in ((270, 480), (1024, 2048)):
        for kind in ("continuous", "quantised", "gated"):
            gt, pred, uncert, count = maps(shape, 3, kind)
            kw = dict(count=count, min_count=3.0) if kind == "gated" else {}
            want = M.compute_uncertainty_metrics(gt, pred, uncert, min_depth_eval=MIN_DEPTH, max_depth_eval=MAX_DEPTH, levels=LEVELS, curves=True, **kw)
            d = {k: torch.from_numpy(v).cuda() for k, v in dict(gt=gt, pred=pred, uncert=uncert, **({"count": count} if kw else {})).items()}
            got = M.compute_uncertainty_metrics_fused(min_count=kw.get("min_count", 0), min_depth_eval=MIN_DEPTH, max_depth_eval=MAX_DEPTH,
                                                      levels=LEVELS, curves=True, **d)
            exact = exact and np.array_equal(got["thresholds"], want["thresholds"]) and np.array_equal(got["kept_count"], want["kept_count"])
            worst[f"{kind}{shape[0]}x{shape[1]}"] = rel_deviation(got, want)
    return dict(bound=1e-9, thresholds_and_counts_equal=bool(exact), max_rel_deviation=float(f"{max(worst.values()):.3e}"),
                per_case={k: float(f"{v:.3e}") for k, v in worst.items()})


def step_size(step, reps):
    from patchrefinerv2_amd import lib, metrics as M
    shape = SIZES[step]
    gt, pred, uncert, count = (torch.from_numpy(a).cuda() for a in maps(shape, 1))
    min_count = 3.0

    def new():
        return M.compute_uncertainty_metrics_fused(gt, pred, uncert, count, min_count, MIN_DEPTH, MAX_DEPTH, LEVELS)

    def base():
        return uncert_torch(gt, pred, uncert, count, min_count, MIN_DEPTH, MAX_DEPTH, LEVELS)
    a, b = new(), base()
    agree = max(abs(a[k] - b[k]) for k in b)
    new_ms = wall_ms(new, reps)
    return dict(shape=list(shape), levels=LEVELS, new_ms=new_ms, torch_ms=wall_ms(base, 5, warm=1), new_alloc_bytes=alloc_bytes(new),
                torch_alloc_bytes=alloc_bytes(base), workspace_bytes=int(lib.load().prv2_sparsify_workspace_bytes(1, *shape, LEVELS)),
                key_map_bytes=13 * shape[0] * shape[1], max_abs_diff_new_vs_torch=float(f"{agree:.3e}"), scores={k: float(f"{v:.6g}") for k, v in a.items()})


def write_u4k_tree(root, n, shape):
    """<root>/<scene>/Image0/<n>.raw (BGR bytes), Disp0/<n>.npy, Extrinsics0|1/<n>.txt and splits/val.txt (u4k_dataset.py's layout)"""
    h, w = shape
    os.makedirs(os.path.join(root, "splits"), exist_ok=True)
    lines = []
    for k in range(n):
        scene, num = "00001", f"{k:05d}"
        for sub in ("Image0", "Disp0", "Extrinsics0", "Extrinsics1"):
            os.makedirs(os.path.join(root, scene, sub), exist_ok=True)
        np.random.default_rng(k).integers(0, 256, (h, w, 3), dtype=np.uint8).tofile(os.path.join(root, scene, "Image0", f"{num}.raw"))
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        disp = 20.0 + 30.0 * (x > w * 0.4 + 7 * k) + 12.0 * (np.hypot(x - w * 0.6, y - h * 0.5) < h * 0.25) + 0.2 * np.sin(y / 5.0)
        disp[:2] = 0.0
        np.save(os.path.join(root, scene, "Disp0", f"{num}.npy"), disp.astype(np.float32))
        for cam, tx in (("Extrinsics0", 0.25), ("Extrinsics1", 0.6)):
            with open(os.path.join(root, scene, cam, f"{num}.txt"), "w") as f:
                f.write(f"480.0 0.0 {w / 2} 0.0 480.0 {h / 2} 0.0 0.0 1.0\n1.0 0.0 0.0 {tx} 0.0 1.0 0.0 0.0 0.0 0.0 1.0 0.0\n")
        lines.append(f"{scene}/Image0/{num}.png {scene}/Image1/{num}.png {scene}/Disp0/{num}.npy {scene}/Disp1/{num}.npy")
    split = os.path.join(root, "splits", "val.txt")
    with open(split, "w") as f:
        f.write("\n".join(lines) + "\n")
    return split


def step_tester(n_maps):
    from patchrefinerv2_amd import tester  # noqa: F401  (registers the datasets)
    from patchrefinerv2_amd.registry import DATASETS
    w, model = EB.workload_model()
    with tempfile.TemporaryDirectory() as root:
        split = write_u4k_tree(root, n_maps, tuple(w["raw"]))
        ds = DATASETS.build(dict(type="UnrealStereo4kDataset", mode="infer", data_root=root, split=split, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH,
                                 transform_cfg=dict(network_process_size=[384, 512]), image_raw_shape=list(w["raw"])))
        out = {}
        for tag, flag in (("uncert_off", False), ("uncert_on", True)):
            out[tag], res, t = EB.timed_maps_s(model, ds, w, n_maps, method="generate_pl", uncert_metrics=flag)
            if flag:
                out["last_eval"] = {k: float(f"{v:.6g}") for k, v in t.last_eval.items()}
                assert all("uncert_metrics" in r for r in res)
        ds.close()
    return dict(workload=EB.WORKLOAD, maps=n_maps, mode=w["mode"], **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--maps", type=int, default=3)
    ap.add_argument("--skip-tester", action="store_true")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uncert_eval.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, ROOT)
        EB.begin_step()
        if a.step == "deviation":
            res = step_deviation()
        elif a.step == "tester":
            res = step_tester(a.maps)
        else:
            res = step_size(a.step, a.reps)
        return EB.end_step(res)
    out = EB.run_steps(__file__, [s for s in STEPS if not (a.skip_tester and s == "tester")], a.step_timeout, ["--reps", a.reps, "--maps", a.maps])
    if "tester" in out:
        t = out["tester"]
        t["uncert_overhead_pct"] = round(100 * (t["uncert_off"] / t["uncert_on"] - 1), 2)
    # the figure tests/test_uncert_eval_gpu.py asserts four times of (measured by that file's own cases, recorded there)
    m = re.search(r"^MEASURED = ([0-9.e+-]+)", open(os.path.join(ROOT, "tests", "test_uncert_eval_gpu.py")).read(), flags=re.M)
    if m:
        out["tests"] = dict(measured_rel_deviation=float(m.group(1)), asserted_rtol=4 * float(m.group(1)), cap=1e-9)
    return EB.report(out, a.out)


if __name__ == "__main__":
    sys.exit(main())
