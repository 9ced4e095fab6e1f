#!/usr/bin/env python
"""Frames per forward call: throughput of one GPU at B = 1, 2, 4, 8 frames per call.

    python tools/bench_frame_batch.py --workload v1_dav2s_1080p_m1 [--batches 1 2 4 8] [--steps 5] [--warmup 2] [--prec f16f6]

The model is built the way bench.py builds it (synthetic weights, the workload's max_batch, 3 streams); every timed call gets B
distinct seeded frames, and the loop announces the next batch (``next_image_lr``) like a frame loop does.  Timed with device events
after the warm-up calls.  One JSON line per B: frames/s, ms per frame, peak torch.cuda.max_memory_allocated, and whether the B-frame
outputs (depth + coarse prediction) were bit-equal to calling the same frames one at a time (B = 1).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default=None)
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 2, 4, 8])
    ap.add_argument("--steps", type=int, default=5, help="timed calls per B")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prec", default="f16f6", choices=["f32", "bf16x3", "f16f6"])
    ap.add_argument("--streams", type=int, default=3)
    ap.add_argument("--max-batch", type=int, default=None)
    ap.add_argument("--no-check", action="store_true", help="skip the bit-equality check against B = 1")
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
    bmax = max(args.batches)

    def image(i):
        return torch.rand(1, 3, *w["raw"], generator=torch.Generator().manual_seed(1000 + i)).to(dev)

    pool = torch.cat([image(i) for i in range(2 * bmax)])  # two batches of distinct frames at the largest B, resident
    pool_lr = model.resizer(pool)

    def call(lo, B, nxt=None, keep=False, views=None):
        """frames lo .. lo + B - 1 of the pool in one call, frame f's plan seeded with 621 + its pool index"""
        hr, lr = views[lo] if views is not None else (pool[lo:lo + B], pool_lr[lo:lo + B])
        d, log = model(mode="infer", cai_mode=w["mode"], process_num=4, tile_cfg=tile_cfg, image_lr=lr, image_hr=hr,
                       frame_seeds=[621 + lo + f for f in range(B)], return_device=True, next_image_lr=nxt)
        if keep:
            return d.clone(), log["coarse_prediction"].clone()
        return None

    ref = None
    if not args.no_check:  # every pool frame alone (B = 1), the reference of the bit-equality check
        ref = [call(i, 1, keep=True) for i in range(2 * bmax)]
    for B in args.batches:
        starts = [0, bmax]  # the batches a call sees alternate between two sets of distinct frames; the next one is announced
        # (one tensor object per batch: the model picks an announced batch up by identity)
        views = {lo: (pool[lo:lo + B], pool_lr[lo:lo + B]) for lo in starts}

        def step(i, last=False):
            lo = starts[i % len(starts)]
            nlo = starts[(i + 1) % len(starts)]
            return call(lo, B, None if last else views[nlo][1], views=views)
        for i in range(args.warmup):
            step(i)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            step(i, last=i == args.steps - 1)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        peak = torch.cuda.max_memory_allocated(dev)
        equal = None
        if ref is not None:
            equal = True
            for lo in starts:
                d, cp = call(lo, B, keep=True)
                equal = equal and torch.equal(d, torch.cat([ref[lo + f][0] for f in range(B)])) and \
                    torch.equal(cp, torch.cat([ref[lo + f][1] for f in range(B)]))
        frames = B * args.steps
        print(json.dumps(dict(workload=name, prec=args.prec, frames_per_call=B, frames_per_s=round(1000.0 * frames / ms, 3),
                              ms_per_frame=round(ms / frames, 4), peak_mem_gb=round(peak / 2 ** 30, 3), bit_equal_to_b1=equal,
                              steps=args.steps, warmup=args.warmup, max_batch=mb, streams=args.streams)), flush=True)


if __name__ == "__main__":
    main()
