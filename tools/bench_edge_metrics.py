#!/usr/bin/env python
"""Edge-aware evaluation cost: one JSON line.

  python tools/bench_edge_metrics.py [--reps 20] [--maps 4] [--skip-tester]

- ``device_ms`` / ``host_ms``: the full boundary evaluation of one frame at 1080p and 4K -- Canny of the log GT and of the log
  prediction, two distance transforms, two 5 x 5 dilations and the statistics (metrics.extract_edges_device +
  compute_boundary_metrics_device against metrics.extract_edges + compute_boundary_metrics).  Device: median of ``--reps`` timed
  calls between HIP events, after a warm-up; host: median of 3.
- ``tester_maps_s``: Tester.run on v2_zoe_4k_r32 (synthetic weights, f16f6, 4K ground truth) with and without ``edge_metrics``.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth_pair(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    gt = 3.0 + 2.0 * (x > 0.45 * w) + 1.5 * (np.hypot(x - 0.25 * w, y - 0.5 * h) < 0.2 * h) + 0.2 * np.sin(y / 37.0) * np.cos(x / 53.0)
    pred = gt * (1 + 0.02 * np.sin(x / 11.0)) + 0.01 * rng.standard_normal(gt.shape)
    return gt.astype(np.float32), pred.astype(np.float32)


def device_ms(gt, pred, reps):
    from patchrefinerv2_amd import metrics as M
    g, p = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()

    def once():
        ge, pe = M.extract_edges_device(g, "log"), M.extract_edges_device(p, "log")
        return M.compute_boundary_metrics_device(ge, pe, (g > 1e-3) & (g < 80))
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        once()  # (ends with the D2H of the scalars)
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def host_ms(gt, pred):
    from patchrefinerv2_amd import metrics as M
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        M.compute_boundary_metrics(M.extract_edges(gt, "log"), M.extract_edges(pred, "log"), (gt > 1e-3) & (gt < 80))
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def tester_maps_s(n_maps, edge_metrics, model=None):
    from patchrefinerv2_amd import models, weights as W  # noqa: F401  (registers the model classes)
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.tester import ImageDataset, RunnerInfo, Tester
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    name = "v2_zoe_4k_r32"
    w = WORKLOADS[name]
    if model is None:
        model = build_model(model_config(name, prec="f16f6", max_batch=int(w.get("max_batch", 41)), n_streams=3))
        model.load_state_dict(W.synth_state_dict(state_spec(name), seed=0), strict=True)
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "imgs"))
        os.makedirs(os.path.join(d, "gt"))
        for i in range(n_maps):
            np.save(os.path.join(d, "imgs", f"f{i}.npy"), np.random.RandomState(i).rand(270, 480, 3).astype(np.float32))
            np.save(os.path.join(d, "gt", f"f{i}.npy"), synth_pair(*w["raw"], seed=i)[0])
        ds = ImageDataset(os.path.join(d, "imgs"), gt_dir=os.path.join(d, "gt"), image_resolution=w["raw"], edge_metrics=edge_metrics)
        t = Tester(None, RunnerInfo(), ds, model)
        run = lambda: t.run(cai_mode=w["mode"], image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621)  # noqa: E731
        run()  # warm-up (kernels, allocator, hipGraphs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        return n_maps / (time.perf_counter() - t0), model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--maps", type=int, default=4)
    ap.add_argument("--skip-tester", action="store_true")
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    from patchrefinerv2_amd import lib
    lib.load()
    out = dict(device_ms={}, host_ms={})
    for tag, (h, w) in (("1080p", (1080, 1920)), ("4k", (2160, 3840))):
        gt, pred = synth_pair(h, w)
        out["device_ms"][tag] = round(device_ms(gt, pred, a.reps), 3)
        out["host_ms"][tag] = round(host_ms(gt, pred), 1)
    if not a.skip_tester:
        base, model = tester_maps_s(a.maps, False)
        edge, _ = tester_maps_s(a.maps, True, model)
        out["tester_maps_s"] = dict(workload="v2_zoe_4k_r32", maps=a.maps, plain=round(base, 3), edge_metrics=round(edge, 3),
                                    overhead_pct=round(100 * (base / edge - 1), 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
