#!/usr/bin/env python
"""Cost of the stereo export (--save-stereo; csrc/stereo.hip, patchrefinerv2_amd/output.py): one JSON line (also written to ``--out``,
default profiles/stereo_export.json).

  python tools/bench_stereo.py [--reps 10] [--maps 2] [--skip-tester] [--baseline-tree DIR --runs 3] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- steps ``4k`` (2160 x 3840) and ``1080p`` (1080 x 1920), on the synthetic depth map and image of tools/bench_geometry.py (camera of a
  60 degree field of view, eyes 0.065 m apart, parallel axes), for the layouts ``right`` and ``sbs``; wall-clock medians per frame, no
  file written on either side:
    ``kernels_ms``  ops.stereo_rows alone (one launch: scatter, fill, gather, scanlines);
    ``device_ms``   what OutputStage.submit_geometry(stereo=...) does up to the writer: the kernel and the copy of the scanline buffer
                    into pinned memory;
    ``host_ms``     the numpy host route of the same commit (the specification, not the code under test): the fp32 map copied to the
                    host, stereo_image_host;
    ``d2h_bytes_*`` bytes copied device -> host per frame on either route; ``holes``: the share of the view's pixels the fill made;
    ``equal``: the two routes' pixels are the same.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over ``--maps`` synthetic images with --save
  --device-output: without and with --save-stereo (right and sbs); files go to a temporary directory (the disk is part of the
  figure) and are on disk when the clock stops.
- step ``baseline`` (with ``--baseline-tree DIR``, a built checkout of the commit to compare with): Tester.run maps/s of the paths this
  export does not touch -- no save, and --save --device-output --save-ply -- ``--runs`` times on this tree and on that one, in
  separate processes.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from bench_geometry import SIZES, _rates, synth  # noqa: E402
from evalbench import wall_ms  # noqa: E402

STEPS = ("4k", "1080p", "tester", "baseline", "baseline_other")
BASELINE = 0.065


def step_size(step, reps):
    from patchrefinerv2_amd import ops, output as O
    h, w = SIZES[step]
    depth, image = synth(h, w)
    k = O.camera_intrinsics((h, w), (h, w))
    d, img = torch.from_numpy(depth).cuda()[None], torch.from_numpy(image).cuda()[None]
    src, _ = ops.stereo_source(d, k, BASELINE)
    res = dict(shape=[h, w], baseline=BASELINE, holes=round(float((src < 0).float().mean()), 5))
    for layout in ("right", "sbs"):
        wout = w * (2 if layout == "sbs" else 1)
        pinned = torch.empty((ops.L.load().prv2_rows_bytes(h, wout, 3),), dtype=torch.uint8, pin_memory=True)

        def kernels():
            return ops.stereo_rows(d, img, k, BASELINE, layout=layout)

        def device():
            pinned.copy_(kernels()[0], non_blocking=True)
            torch.cuda.current_stream().synchronize()

        def host():
            return O.stereo_image_host(d[0].cpu().numpy(), image, k, BASELINE, layout=layout)
        device()
        got = pinned.numpy()[:h * (1 + 3 * wout)].reshape(h, 1 + 3 * wout)[:, 1:].reshape(h, wout, 3)
        equal = np.array_equal(got, host())
        res[layout] = dict(kernels_ms=wall_ms(kernels, reps), device_ms=wall_ms(device, reps), host_ms=wall_ms(host, 3, warm=1),
                           d2h_bytes_device=int(pinned.numel()), d2h_bytes_host=4 * h * w, equal=bool(equal))
    return res


def step_tester(n_maps):
    dev = dict(save=True, device_output=True)
    return _rates(dict(device=dev, device_stereo=dict(dev, save_stereo=True), device_stereo_sbs=dict(dev, save_stereo=True, stereo_layout="sbs")),
                  n_maps)


def step_baseline(n_maps, runs):
    return _rates(dict(no_save={}, device_ply=dict(save=True, device_output=True, save_ply=True)), n_maps, runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maps", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3, help="--baseline-tree: timed runs per case and tree")
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--baseline-tree", default=None, help="a built checkout to compare Tester.run without the new flag with")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stereo_export.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.baseline_tree) if a.step == "baseline_other" else ROOT)
        EB.begin_step()
        if a.step in SIZES:
            res = step_size(a.step, a.reps)
        elif a.step == "tester":
            res = step_tester(a.maps)
        else:
            res = step_baseline(a.maps, a.runs)
        return EB.end_step(res)
    steps = [s for s in STEPS if not (a.skip_tester and s == "tester") and (a.baseline_tree or not s.startswith("baseline"))]
    args = ["--reps", a.reps, "--maps", a.maps, "--runs", a.runs] + (["--baseline-tree", a.baseline_tree] if a.baseline_tree else [])
    out = EB.run_steps(__file__, steps, a.step_timeout, args)
    if "baseline" in out:
        out["baseline"] = dict(this_tree=out.pop("baseline"), other_tree=out.pop("baseline_other"))
    return EB.report(out, a.out)


if __name__ == "__main__":
    sys.exit(main())
