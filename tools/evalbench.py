"""What the evaluation benches share (bench_u4k_eval, bench_general_gt, bench_eth_eval, bench_ssi_eval, bench_uncert_eval, bench_geometry): the two
per-call measurements, the timed Tester run on the flagship workload, and the runner that gives every GPU step a process of its own.
The package is imported inside the functions: a tool decides first which tree's package it measures (``sys.path``)."""
from __future__ import annotations

import json
import os
import statistics
import subprocess
import sys
import time

import torch

WORKLOAD = "v2_zoe_4k_r32"


def wall_ms(fn, reps, warm=2):
    """median wall-clock milliseconds of ``reps`` calls with a device synchronisation at each end, after ``warm`` calls"""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


def alloc_bytes(fn):
    """device bytes the caching allocator hands out during one call"""
    torch.cuda.synchronize()
    key = "allocated_bytes.all.allocated"
    b0 = torch.cuda.memory_stats()[key]
    out = fn()
    torch.cuda.synchronize()
    del out
    return int(torch.cuda.memory_stats()[key] - b0)


class NoGroundTruth:
    """the dataset with ``depth_gt`` / ``boundary`` dropped from its items: Tester.run then scores nothing"""

    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getattr__(self, k):
        return getattr(self.ds, k)

    def __getitem__(self, i):
        return {k: v for k, v in self.ds[i].items() if k not in ("depth_gt", "boundary")}


def workload_model():
    """-> (the flagship workload's entry, its model with synthetic weights, f16f6)"""
    from patchrefinerv2_amd import models, weights as W  # noqa: F401  (registers the model classes)
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    w = WORKLOADS[WORKLOAD]
    model = build_model(model_config(WORKLOAD, prec="f16f6", max_batch=int(w.get("max_batch", 41)), n_streams=3))
    model.load_state_dict(W.synth_state_dict(state_spec(WORKLOAD), seed=0), strict=True)
    return w, model


def timed_maps_s(model, ds, w, n_maps, method="run", info=None, **kw):
    """``Tester.<method>`` over ``ds`` with the workload's arguments, once to warm up (kernels, allocator, hipGraphs, page cache) and once
    timed -> (maps/s, the timed call's results, the Tester).  ``info``: the RunnerInfo (default: one process, nothing saved)"""
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    t = Tester(None, info or RunnerInfo(rank=0, world_size=1), ds, model)

    def run():
        return getattr(t, method)(cai_mode=w["mode"], image_raw_shape=w["raw"], patch_split_num=w["split"], seed=621, **kw)
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = run()
    torch.cuda.synchronize()
    return round(n_maps / (time.perf_counter() - t0), 3), res, t


def gt_pair_maps_s(model, ds, w, n_maps):
    """Tester.run maps/s with ground truth (decoded and scored) and with it dropped from the items (nothing scored) ->
    (dict(overhead_pct, with_gt, without_gt), the number of keys of the scored run's ``last_eval``)"""
    with_gt, res, t = timed_maps_s(model, ds, w, n_maps)
    assert "metrics" in res[0]
    without_gt, res, _ = timed_maps_s(model, NoGroundTruth(ds), w, n_maps)
    assert "metrics" not in res[0]
    return dict(overhead_pct=round(100 * (without_gt / with_gt - 1), 2), with_gt=with_gt, without_gt=without_gt), len(t.last_eval)


def begin_step():
    """what a process does before it measures"""
    torch.set_grad_enabled(False)
    from patchrefinerv2_amd import lib
    lib.load()


def add_step_arguments(ap, steps):
    ap.add_argument("--step-timeout", type=int, default=280, help="seconds each GPU step may take")
    ap.add_argument("--step", choices=steps, default=None, help="(internal) run one step in this process and print its JSON")


def end_step(res):
    print("RESULT " + json.dumps(res))
    return 0


def run_steps(script, steps, timeout, args):
    """every step in a child process of its own under a time limit: ``python script --step S *args`` -> {step: what it gave to
    ``end_step``}.  The first step that does not exit with status 0 (a fault, an abort or the time limit) ends the tool with that
    status: nothing more is started on the GPU."""
    out = {}
    for step in steps:
        cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(script), "--step", step] + [str(a) for a in args]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:] + f"\nstep {step} exited with status {r.returncode}: stopping\n")
            sys.exit(r.returncode)
        out[step] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        sys.stderr.write(f"step {step}: done\n")  # (a sign of life between steps; the result is the one JSON line at the end)
    return out


def report(out, path):
    """the tool's one JSON line, printed and (``path``) written"""
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
    return 0
