#!/usr/bin/env python
"""Cost of the overlap statistics: throughput with and without ``return_uncertainty`` on one GPU.

    python tools/bench_uncertainty.py --workload v2_zoe_4k_r32 [--batches 1 4] [--steps 5] [--warmup 2] [--reps 3] [--prec f16f6]

The model is built the way bench.py builds it (synthetic weights, the workload's max_batch, 3 streams).  For each B, ``reps`` rounds
each time ``steps`` calls of B seeded frames without and with ``return_uncertainty=True`` (the order alternates from round to round),
with device events after ``warmup`` calls of each kind; the maps stay on the device (``return_device=True``).  One JSON line per B:
the median maps/s of either kind, the overhead of the statistics from the medians, and whether the depth of the two kinds was
bit-equal on the same frames and tile plans.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default=None)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 4])
    ap.add_argument("--steps", type=int, default=5, help="timed calls per round and kind")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3, help="rounds per B (the medians are taken over them)")
    ap.add_argument("--prec", default="f16f6", choices=["f32", "bf16x3", "f16f6"])
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=None)
    args = ap.parse_args()

    from patchrefinerv2_amd import models, weights as W  # noqa: F401
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.workloads import DEFAULT_WORKLOAD, WORKLOADS, model_config, state_spec
    name = args.workload or DEFAULT_WORKLOAD
    w = WORKLOADS[name]
    mb = args.max_batch if args.max_batch is not None else int(w.get("max_batch", 41))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    mc = model_config(name, prec=args.prec, max_batch=mb, n_streams=args.streams)
    mc["config"]["device"] = str(dev)
    model = build_model(mc)
    model.load_state_dict(W.synth_state_dict(state_spec(name), seed=0), strict=True)
    tile_cfg = dict(image_raw_shape=w["raw"], patch_split_num=w["split"])

    for B in args.batches:
        hr = torch.cat([torch.rand(1, 3, *w["raw"], generator=torch.Generator().manual_seed(1000 + f)) for f in range(B)]).to(dev)
        lr = model.resizer(hr)
        seeds = [621 + f for f in range(B)]

        def call(stats):
            return model(mode="infer", cai_mode=w["mode"], process_num=4, tile_cfg=tile_cfg, image_lr=lr, image_hr=hr, frame_seeds=seeds,
                         return_device=True, return_uncertainty=stats)

        for stats in (False, True):
            for _ in range(args.warmup):
                call(stats)
        rates = {False: [], True: []}
        for r in range(args.reps):
            for stats in ((False, True) if r % 2 == 0 else (True, False)):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    call(stats)
                e1.record()
                torch.cuda.synchronize()
                rates[stats].append(1000.0 * B * args.steps / e0.elapsed_time(e1))
        d_off, _ = call(False)
        d_off = d_off.clone()
        d_on, log = call(True)
        equal = bool(torch.equal(d_off, d_on))
        off, on = statistics.median(rates[False]), statistics.median(rates[True])
        print(json.dumps(dict(workload=name, prec=args.prec, frames_per_call=B, maps_per_s=round(off, 3), maps_per_s_uncertainty=round(on, 3),
                              overhead_pct=round(100.0 * (off / on - 1.0), 2), depth_bit_equal=equal,
                              max_count=float(log["count_map"].max()), runs=dict(off=[round(x, 3) for x in rates[False]],
                                                                                 on=[round(x, 3) for x in rates[True]]),
                              steps=args.steps, warmup=args.warmup, reps=args.reps, max_batch=mb, streams=args.streams)), flush=True)


if __name__ == "__main__":
    main()
