#!/usr/bin/env python
"""Cost of the temporal stabiliser (--temporal-stabilize; csrc/temporal.hip, patchrefinerv2_amd/temporal.py): one JSON line (also
written to ``--out``, default profiles/temporal.json).

  python tools/bench_temporal.py [--reps 20] [--frames 32] [--maps 3] [--runs 3] [--skip-tester] [--baseline-tree DIR] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- steps ``1080p`` (1080 x 1920) and ``4k`` (2160 x 3840): a jittered static scene with an image of the map's size, 8 frames per call
  in steady state (a state is present); wall-clock medians:
    ``step_ms_per_frame``   ops.temporal_step (four launches per frame), per frame;
    ``bytes_per_frame``     what the step moves per frame, from the shapes: the fit pass reads x, y (4 + 4 bytes a pixel), the
                            previous luma (1) and the image (12) and writes the luma (1); the apply pass reads x, y, both lumas
                            (4 + 4 + 1 + 1) and writes out (4) -- 36 bytes a pixel, plus 4 when a call's last frame also writes the
                            state (here one frame in 8: 36.5);
    ``step_gb_s``           those bytes over the step's time;
    ``copy_gb_s``           the yardstick: a torch device-to-device copy that moves the same byte count (half read, half written) on
                            the same box, timed the same way;
    ``stats_d2h_ms``        TemporalStabilizer.step per frame, i.e. with the one copy of the stats rows to the host that ends a call;
    ``host_ms``             temporal_step_host (the numpy specification) for one frame;
    ``equal``               the device's bits equal the specification's on that frame.
- step ``tester_1080p``: Tester.run frames/s on v1_dav2s_1080p_m1 (synthetic weights, f16f6, nothing saved) with --frame-batch 8 over
  ``--frames`` images, without and with the flag, ``--runs`` timed runs each, alternating; ``tester_4k``: the same on v2_zoe_4k_r32,
  one frame per call, ``--maps`` images.
- steps ``baseline_*`` (with ``--baseline-tree DIR``, a built checkout of the commit to compare with): the runs without the flag on
  that tree, in processes of their own.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from evalbench import wall_ms  # noqa: E402

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
TESTER = {"tester_1080p": ("v1_dav2s_1080p_m1", 8), "tester_4k": ("v2_zoe_4k_r32", 1)}
STEPS = ("1080p", "4k", "tester_1080p", "tester_4k", "baseline_1080p", "baseline_4k")
CALL = 8  # frames per call of the size steps


def synth(h, w, frames, seed=0):
    """a static scene under a jittering estimator (+-5 % scale, +-0.03 m shift, 2 mm noise) and a textured image whose grey levels move
    by one or two from frame to frame -> (depth fp32 [frames, h, w], image fp32 [frames, 3, h, w]) on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32), indexing="ij")
    base = 2.0 + 6.0 * x / w + 0.5 * torch.sin(y / 37.0)
    tex = torch.rand((3, h, w), device="cuda", generator=g) * 0.6 + 0.2
    rs = np.random.RandomState(seed)
    d = torch.stack([base * (1.0 + rs.uniform(-0.05, 0.05)) + rs.uniform(-0.03, 0.03) + 0.002 * torch.randn((h, w), device="cuda", generator=g)
                     for _ in range(frames)])
    img = torch.stack([(tex + torch.randint(-2, 3, (1, h, w), device="cuda", generator=g) / 255.0).clamp(0, 1) for _ in range(frames)])
    return d.contiguous(), img.contiguous()


def step_size(step, reps):
    from patchrefinerv2_amd import ops, temporal as T
    h, w = SIZES[step]
    d, img = synth(h, w, CALL)
    state, luma = torch.empty((h, w), device="cuda"), torch.empty((2, h, w), dtype=torch.uint8, device="cuda")
    ops.temporal_step(d, img, state, luma[0], luma[1], False)  # (8 frames: the state leaves in luma[0])

    def step():
        return ops.temporal_step(d, img, state, luma[0], luma[1], True)
    nbytes = int(h * w * (36 * CALL + 4))  # of one call
    src, dst = torch.empty((nbytes // 2,), dtype=torch.uint8, device="cuda"), torch.empty((nbytes // 2,), dtype=torch.uint8, device="cuda")
    stab = T.TemporalStabilizer()
    stab.step(d[:, None], img)
    step_ms, copy_ms = wall_ms(step, reps), wall_ms(lambda: dst.copy_(src), reps)
    full_ms = wall_ms(lambda: stab.step(d[:, None], img), reps)
    # one frame against the specification (and its time)
    x0, x1, i0, i1 = d[0].cpu().numpy(), d[1].cpu().numpy(), img[0].cpu().numpy(), img[1].cpu().numpy()
    _, st, _ = T.temporal_step_host(x0, i0, None)
    want, _, row = T.temporal_step_host(x1, i1, st)
    host_ms = wall_ms(lambda: T.temporal_step_host(x1, i1, st), 3, warm=1)
    s2, l2 = torch.empty((h, w), device="cuda"), torch.empty((2, h, w), dtype=torch.uint8, device="cuda")
    out, stats = ops.temporal_step(d[:2], img[:2], s2, l2[0], l2[1], False)
    equal = out[1].cpu().numpy().tobytes() == want.tobytes() and np.array_equal(stats[1].cpu().numpy(), row)
    sd = T.stats_dict(row, h * w)
    return dict(shape=[h, w], frames_per_call=CALL, step_ms_per_frame=round(step_ms / CALL, 4), bytes_per_frame=nbytes // CALL,
                step_gb_s=round(nbytes / step_ms / 1e6, 1), copy_gb_s=round(nbytes / copy_ms / 1e6, 1), copy_ms_same_bytes=round(copy_ms / CALL, 4),
                stats_d2h_ms=round(full_ms / CALL, 4), host_ms=host_ms, equal=bool(equal), fitted=sd["fitted"],
                static_fraction=round(sd["static_fraction"], 4), change_before=sd["change_before"], change_after=sd["change_after"])


def _model(name):
    from patchrefinerv2_amd import models, weights as W  # noqa: F401  (registers the model classes)
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    w = WORKLOADS[name]
    model = build_model(model_config(name, prec="f16f6", max_batch=int(w.get("max_batch", 41)), n_streams=3))
    model.load_state_dict(W.synth_state_dict(state_spec(name), seed=0), strict=True)
    return w, model


def step_tester(step, n, runs, flag):
    """Tester.run frames/s, nothing saved: ``runs`` timed runs without and (``flag``) with the stabiliser, alternating"""
    from patchrefinerv2_amd.tester import ImageDataset, RunnerInfo
    name, fb = TESTER[step.replace("baseline", "tester")]
    w, model = _model(name)
    cases = dict(off={}, **(dict(on=dict(temporal_stabilize=True)) if flag else {}))
    out = {k: [] for k in cases}
    with tempfile.TemporaryDirectory() as root:
        imgs = os.path.join(root, "imgs")
        os.makedirs(imgs)
        tex = np.random.RandomState(0).rand(270, 480, 3).astype(np.float32)
        for i in range(n):  # a nearly static clip
            np.save(os.path.join(imgs, f"f{i:03d}.npy"), np.clip(tex + np.random.RandomState(i).randint(-1, 2, (270, 480, 1)) / 255.0, 0, 1).astype(np.float32))
        ds = ImageDataset(imgs, image_resolution=w["raw"])
        temporal = None
        for _ in range(runs):
            for k, kw in cases.items():
                rate, res, _ = EB.timed_maps_s(model, ds, w, n, info=RunnerInfo(rank=0, world_size=1, **kw), frame_batch=fb)
                out[k].append(rate)
                if k == "on":
                    temporal = [r["temporal"] for r in res]
    res = dict(workload=name, frames=n, frame_batch=fb, mode=w["mode"], **out)
    if temporal:
        res.update(resets=sum(t["reset"] for t in temporal), static_fraction=round(float(np.mean([t["static_fraction"] for t in temporal[1:]])), 4))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=32, help="tester_1080p: frames of the clip")
    ap.add_argument("--maps", type=int, default=3, help="tester_4k: frames of the clip")
    ap.add_argument("--runs", type=int, default=3, help="timed runs per case")
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--baseline-tree", default=None, help="a built checkout to compare Tester.run without the flag with")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.baseline_tree) if a.step.startswith("baseline") else ROOT)
        EB.begin_step()
        if a.step in SIZES:
            res = step_size(a.step, a.reps)
        else:
            res = step_tester(a.step, a.frames if a.step.endswith("1080p") else a.maps, a.runs, flag=a.step.startswith("tester"))
        return EB.end_step(res)
    steps = [s for s in STEPS if not (a.skip_tester and s.startswith("tester")) and (a.baseline_tree or not s.startswith("baseline"))]
    args = ["--reps", a.reps, "--frames", a.frames, "--maps", a.maps, "--runs", a.runs] + (["--baseline-tree", a.baseline_tree] if a.baseline_tree else [])
    return EB.report(EB.run_steps(__file__, steps, a.step_timeout, args), a.out)


if __name__ == "__main__":
    sys.exit(main())
