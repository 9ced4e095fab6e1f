#!/usr/bin/env python
"""Cost and effect of the temporal stabiliser's motion stage (--temporal-stabilize --temporal-motion; csrc/motion.hip,
patchrefinerv2_amd/temporal.py): one JSON line (also written to ``--out``, default profiles/temporal_motion.json).

  python tools/bench_temporal_motion.py [--reps 20] [--frames 32] [--maps 3] [--runs 3] [--skip-tester] [--parent-tree DIR] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- steps ``1080p`` (1080 x 1920) and ``4k`` (2160 x 3840): the jittered scene of tools/bench_temporal.py under a camera that pans by
  (3, -7) pixels per frame (a smoothed texture and the depth map cut from a larger scene), 8 frames per call in steady state (a state
  is present); wall-clock medians of the same process:
    ``plain_ms_per_frame``    ops.temporal_step (four launches per frame);
    ``copy_ms_map_bytes``     the yardstick: a torch device-to-device copy of one frame's map bytes (4 h w read, 4 h w written);
    per R in 4, 8, 16:
    ``step_ms_per_frame``     ops.temporal_motion_step (ten launches per frame);
    ``motion_ms_per_frame``   that minus ``plain_ms_per_frame``: the six motion launches (a difference of two medians, not a kernel
                              time; the launches' own times come from a kernel trace of this step);
    ``sad_bytes_per_frame``   the absolute byte differences the two searches take, from the shapes: nb ((2R + 1)^2 + 1) 64 coarse
                              and nb (49 x 256 + 256) fine for nb blocks;
    ``sad_gbyte_s``           those over ``motion_ms_per_frame``; ``valu_share``: over the packed-SAD issue rate of the vector units
                              (256 CUs x 128 lanes x 4 bytes x 2.4 GHz = 314.6 Tbyte/s);
    ``quality``               TemporalStabilizer over the clip without and with the stage (R = 8): means over the frames after the
                              first of static_fraction, change_before, change_after; with the stage also moving_fraction, mean_dy / dx;
    ``equal``                 the device's bits of one frame (out, both stats rows, the vectors) equal the specification's (1080p only:
                              the specification takes seconds per 4K frame).
- step ``tester_1080p``: Tester.run frames/s on v1_dav2s_1080p_m1 (synthetic weights, f16f6, nothing saved) with --frame-batch 8 over
  ``--frames`` images of a panning clip, with --temporal-stabilize and with --temporal-stabilize --temporal-motion, ``--runs`` timed
  runs each, alternating; ``tester_4k``: the same as maps/s on v2_zoe_4k_r32, one frame per call, ``--maps`` images.
- steps ``parent_*`` / ``this_*`` (with ``--parent-tree DIR``, a built checkout of the parent commit): the unchanged path -- the runs
  with --temporal-stabilize alone on that tree and on this one, in processes of their own, alternating, three of each.
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
from evalbench import wall_ms  # noqa: E402

SIZES = {"4k": (2160, 3840), "1080p": (1080, 1920)}
TESTER = {"1080p": ("v1_dav2s_1080p_m1", 8), "4k": ("v2_zoe_4k_r32", 1)}
AB = tuple(f"{tree}_{size}_{k}" for k in range(3) for size in ("1080p", "4k") for tree in ("parent", "this"))  # alternating
STEPS = ("1080p", "4k", "tester_1080p", "tester_4k") + AB
CALL = 8  # frames per call of the size steps
PAN = (3, -7)
RANGES = (4, 8, 16)
VALU_SAD_BYTES_S = 256 * 128 * 4 * 2.4e9


def synth(h, w, frames, seed=0):
    """bench_temporal.synth's jittering estimator (+-5 % scale, +-0.03 m shift, 2 mm noise) over a scene that pans by PAN per frame: the
    depth map and a 3 x 3-smoothed texture are cut from larger ones -> (depth fp32 [frames, h, w], image fp32 [frames, 3, h, w])"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = 8 * frames
    H, W = h + 2 * m, w + 2 * m
    y, x = torch.meshgrid(torch.arange(H, device="cuda", dtype=torch.float32), torch.arange(W, device="cuda", dtype=torch.float32), indexing="ij")
    base = 2.0 + 6.0 * x / W + 0.5 * torch.sin(y / 37.0)
    tex = F.avg_pool2d(torch.rand((1, 1, H + 2, W + 2), device="cuda", generator=g), 3, stride=1)[0].expand(3, H, W) * 0.8 + 0.1
    rs = np.random.RandomState(seed)
    d, img = [], []
    for t in range(frames):
        y0, x0 = m + PAN[0] * t, m + PAN[1] * t
        d.append(base[y0:y0 + h, x0:x0 + w] * (1.0 + rs.uniform(-0.05, 0.05)) + rs.uniform(-0.03, 0.03) + 0.002 * torch.randn((h, w), device="cuda", generator=g))
        img.append(tex[:, y0:y0 + h, x0:x0 + w])
    return torch.stack(d).contiguous(), torch.stack(img).contiguous()


def sad_bytes(h, w, R):
    nb = -(-h // 16) * -(-w // 16)
    return nb * (((2 * R + 1) ** 2 + 1) * 64 + 49 * 256 + 256)


def step_size(step, reps):
    from patchrefinerv2_amd import ops, temporal as T
    h, w = SIZES[step]
    d, img = synth(h, w, CALL)
    state, luma = torch.empty((h, w), device="cuda"), torch.empty((2, h, w), dtype=torch.uint8, device="cuda")
    ops.temporal_step(d, img, state, luma[0], luma[1], False)  # (8 frames: the state leaves in luma[0])
    plain_ms = wall_ms(lambda: ops.temporal_step(d, img, state, luma[0], luma[1], True), reps) / CALL
    src, dst = torch.empty((h, w), device="cuda"), torch.empty((h, w), device="cuda")
    copy_ms = wall_ms(lambda: [dst.copy_(src) for _ in range(CALL)], reps) / CALL
    res = dict(shape=[h, w], frames_per_call=CALL, pan=list(PAN), plain_ms_per_frame=round(plain_ms, 4), copy_ms_map_bytes=round(copy_ms, 4), ranges={})
    for R in RANGES:
        ms = wall_ms(lambda: ops.temporal_motion_step(d, img, state, luma[0], luma[1], True, motion_range=R), reps) / CALL
        motion = ms - plain_ms
        res["ranges"][str(R)] = dict(step_ms_per_frame=round(ms, 4), motion_ms_per_frame=round(motion, 4), sad_bytes_per_frame=sad_bytes(h, w, R),
                                     sad_gbyte_s=round(sad_bytes(h, w, R) / motion / 1e6, 1),
                                     valu_share=round(sad_bytes(h, w, R) / (motion * 1e-3) / VALU_SAD_BYTES_S, 4))
    quality = {}
    for name, kw in (("plain", {}), ("motion", dict(motion=True))):
        stats = T.TemporalStabilizer(**kw).step(d[:, None], img)[1][1:]
        quality[name] = {k: round(float(np.mean([s[k] for s in stats])), 5) for k in ("static_fraction", "change_before", "change_after")}
        if kw:
            quality[name].update({k: round(float(np.mean([s["motion"][k] for s in stats])), 4) for k in ("moving_fraction", "mean_dy", "mean_dx")})
    res["quality"] = quality
    if step == "1080p":  # one frame against the specification
        x0, x1, i0, i1 = d[0].cpu().numpy(), d[1].cpu().numpy(), img[0].cpu().numpy(), img[1].cpu().numpy()
        _, st, _ = T.temporal_step_host(x0, i0, None)
        vec = T.temporal_motion_host(T.luma_host(i1, h, w), st[1], 8)[0]
        want, _, row, mrow = T.temporal_step_host(x1, i1, st, motion_range=8)
        s2, l2 = torch.empty((h, w), device="cuda"), torch.empty((2, h, w), dtype=torch.uint8, device="cuda")
        out, stats, mstats, vecs = ops.temporal_motion_step(d[:2], img[:2], s2, l2[0], l2[1], False, motion_range=8)
        res["equal"] = bool(out[1].cpu().numpy().tobytes() == want.tobytes() and np.array_equal(stats[1].cpu().numpy(), row)
                            and np.array_equal(mstats[1].cpu().numpy(), mrow) and np.array_equal(vecs[1].cpu().numpy(), vec))
    return res


def _model(name):
    from patchrefinerv2_amd import models, weights as W  # noqa: F401  (registers the model classes)
    from patchrefinerv2_amd.registry import build_model
    from patchrefinerv2_amd.workloads import WORKLOADS, model_config, state_spec
    w = WORKLOADS[name]
    model = build_model(model_config(name, prec="f16f6", max_batch=int(w.get("max_batch", 41)), n_streams=3))
    model.load_state_dict(W.synth_state_dict(state_spec(name), seed=0), strict=True)
    return w, model


def step_tester(size, n, runs, cases):
    """Tester.run frames/s over a panning clip, nothing saved: ``runs`` timed runs of every case, alternating"""
    from patchrefinerv2_amd.tester import ImageDataset, RunnerInfo
    name, fb = TESTER[size]
    w, model = _model(name)
    out = {k: [] for k in cases}
    with tempfile.TemporaryDirectory() as root:
        imgs = os.path.join(root, "imgs")
        os.makedirs(imgs)
        big = F.avg_pool2d(torch.rand((1, 1, 272 + 8 * n, 482 + 8 * n), generator=torch.Generator().manual_seed(0)), 3, stride=1)[0, 0].numpy()
        for i in range(n):  # the clip is decoded at 270 x 480 and resized to the workload's raw shape
            y0, x0 = 4 * n + i, 4 * n - 2 * i
            np.save(os.path.join(imgs, f"f{i:03d}.npy"), np.repeat(big[y0:y0 + 270, x0:x0 + 480, None], 3, axis=2).astype(np.float32))
        ds = ImageDataset(imgs, image_resolution=w["raw"])
        temporal = {}
        for _ in range(runs):
            for k, kw in cases.items():
                rate, res, _ = EB.timed_maps_s(model, ds, w, n, info=RunnerInfo(rank=0, world_size=1, **kw), frame_batch=fb)
                out[k].append(rate)
                temporal[k] = [r["temporal"] for r in res]
    res = dict(workload=name, frames=n, frame_batch=fb, mode=w["mode"], **out)
    for k, rows in temporal.items():
        res[k + "_static_fraction"] = round(float(np.mean([t["static_fraction"] for t in rows[1:]])), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=32, help="tester_1080p: frames of the clip")
    ap.add_argument("--maps", type=int, default=3, help="tester_4k: frames of the clip")
    ap.add_argument("--runs", type=int, default=3, help="timed runs per case")
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: the unchanged path (--temporal-stabilize alone) on both trees")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_motion.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.parent_tree) if a.step.startswith("parent") else ROOT)
        EB.begin_step()
        if a.step in SIZES:
            return EB.end_step(step_size(a.step, a.reps))
        size = a.step.split("_")[1]
        n = a.frames if size == "1080p" else a.maps
        if a.step.startswith("tester"):
            return EB.end_step(step_tester(size, n, a.runs, dict(stabilize=dict(temporal_stabilize=True),
                                                                 motion=dict(temporal_stabilize=True, temporal_motion=True))))
        return EB.end_step(step_tester(size, n, 1, dict(stabilize=dict(temporal_stabilize=True))))
    steps = [s for s in STEPS if not (a.skip_tester and s.startswith("tester")) and (a.parent_tree or s not in AB)]
    args = ["--reps", a.reps, "--frames", a.frames, "--maps", a.maps, "--runs", a.runs] + (["--parent-tree", a.parent_tree] if a.parent_tree else [])
    return EB.report(EB.run_steps(__file__, steps, a.step_timeout, args), a.out)


if __name__ == "__main__":
    sys.exit(main())
