#!/usr/bin/env python
"""Cost of the depth-of-field export (--save-bokeh; csrc/bokeh.hip, patchrefinerv2_amd/output.py): one JSON line (also written to
``--out``, default profiles/bokeh_export.json).

  python tools/bench_bokeh.py [--reps 10] [--maps 2] [--skip-tester] [--baseline-tree DIR --runs 3] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

- steps ``4k`` (2160 x 3840) and ``1080p`` (1080 x 1920), on a portrait-like scene (``synth``: a subject 1.5 m away in front of a
  background that recedes from 2 m to 12 m; a camera of a 60 degree field of view, a lens of 0.025 m focused on the subject), at
  max_radius 8, 16 and the cap; wall-clock medians per frame, no file written:
    ``kernels_ms``            ops.bokeh_rows alone (one launch), every tile's walk bounded by the radii in its reach;
    ``kernels_unbounded_ms``  the same kernel with the bound off (prv2_bokeh_tile_bound(0)): every tile walks the full window;
    ``device_ms``             what OutputStage.submit_geometry(bokeh=...) does up to the writer: the kernel and the copy of the scanline
                              buffer into pinned memory;
    ``in_focus_tiles``        the share of the 64 x 16 tiles whose walk is the centre tap alone; ``walked``: the share of the full
                              window's taps the bounded kernel walks; ``gtaps_s``: the full window's taps per second of the unbounded
                              kernel, ``gtaps_s_bounded``: the walked taps per second of the bounded one;
    ``d2h_bytes_*``           bytes copied device -> host per frame on either route;
    ``host_ms`` / ``equal``   1080p at max_radius 8 only, one run: the numpy host route (the specification: the fp32 map copied to the
                              host, bokeh_image_host) and whether the two routes' bytes are the same.  The host is not timed at 4K or
                              at a larger radius: it takes minutes per frame there.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over ``--maps`` synthetic images with --save
  --device-output: without and with --save-bokeh; files go to a temporary directory (the disk is part of the figure) and are on disk
  when the clock stops.
- steps ``baseline`` / ``baseline_other`` (with ``--baseline-tree DIR``, a built checkout of the commit to compare with): Tester.run
  maps/s of the paths this export does not touch -- no save, and --save --device-output -- once per process, ``--runs`` times
  alternating between this tree and that one.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))  # (the package's tree is chosen per step, in main)
import evalbench as EB  # noqa: E402
from bench_geometry import SIZES, _rates  # noqa: E402
from evalbench import wall_ms  # noqa: E402

STEPS = ("4k", "1080p", "tester", "baseline", "baseline_other")
APERTURE = 0.025
TILE = (16, 64)  # rows, columns of a workgroup's tile (csrc/bokeh.hip)


def synth(h, w, seed=0):
    """a subject (a disc, 1.5 m) in front of a background that recedes from 2 m to 12 m, with a little noise; an image of the same size"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    rs = np.random.RandomState(seed)
    d = 2.0 + 10.0 * (x / w) + 0.01 * rs.rand(h, w)
    d[np.hypot(x - w * 0.5, y - h * 0.5) < h * 0.3] = 1.5
    return d.astype(np.float32), rs.rand(3, h, w).astype(np.float32)


def tile_walks(depth, fx, rm):
    """-> Rt of every tile (a device tensor): the window a tile of the kernel walks, from the specification's radii"""
    import torch.nn.functional as F
    from patchrefinerv2_amd import output as O
    zf = O.bokeh_focus_host(depth)
    m = torch.from_numpy(O.bokeh_discs_host(depth, fx, APERTURE, zf, rm)[2]).cuda()[None, None]
    R = int(math.ceil(rm))
    h, w = depth.shape
    pad_b, pad_r = -h % TILE[0], -w % TILE[1]
    m = F.pad(m, (R, R + pad_r, R, R + pad_b), value=0.5)
    mmax = F.max_pool2d(m, kernel_size=(TILE[0] + 2 * R, TILE[1] + 2 * R), stride=TILE)[0, 0]
    return torch.clamp(torch.ceil(mmax + 0.5) - 1, max=R)


def step_size(step, reps):
    from patchrefinerv2_amd import ops, output as O
    lib = ops.L.load()
    h, w = SIZES[step]
    depth, image = synth(h, w)
    k = O.camera_intrinsics((h, w), (h, w))
    d, img = torch.from_numpy(depth).cuda()[None], torch.from_numpy(image).cuda()[None]
    pinned = torch.empty((lib.prv2_rows_bytes(h, w, 3),), dtype=torch.uint8, pin_memory=True)
    res = dict(shape=[h, w], aperture=APERTURE, focus=float(O.bokeh_focus_host(depth)))
    for rm in (8.0, 16.0, float(lib.prv2_bokeh_max_radius())):
        def kernels():
            return ops.bokeh_rows(d, img, k, APERTURE, max_radius=rm)

        def device():
            pinned.copy_(kernels()[0][0], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        rt = tile_walks(depth, k[0], rm)
        full = (2 * math.ceil(rm) + 1) ** 2
        walked = float(((2 * rt + 1) ** 2).mean()) / full
        bounded = wall_ms(kernels, reps)
        assert lib.prv2_bokeh_tile_bound(0) == 1
        try:
            unbounded = wall_ms(kernels, reps)
        finally:
            lib.prv2_bokeh_tile_bound(1)
        r = dict(kernels_ms=bounded, kernels_unbounded_ms=unbounded, device_ms=wall_ms(device, reps),
                 in_focus_tiles=round(float((rt == 0).float().mean()), 4), walked=round(walked, 4),
                 gtaps_s=round(h * w * full / unbounded / 1e6, 1), gtaps_s_bounded=round(h * w * full * walked / bounded / 1e6, 1),
                 d2h_bytes_device=int(pinned.numel()) + 4, d2h_bytes_host=4 * h * w)
        if step == "1080p" and rm == 8.0:  # the specification, once: minutes per frame at 4K or at a larger radius
            device()
            got = pinned.numpy()[:h * (1 + 3 * w)].reshape(h, 1 + 3 * w)[:, 1:].reshape(h, w, 3).copy()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = O.bokeh_image_host(d[0].cpu().numpy(), image, k, APERTURE, max_radius=rm)
            r.update(host_ms=round((time.perf_counter() - t0) * 1e3, 1), equal=bool(np.array_equal(got, want)))
        res[f"r{rm:g}"] = r
    return res


def step_tester(n_maps):
    dev = dict(save=True, device_output=True)
    return _rates(dict(device=dev, device_bokeh=dict(dev, save_bokeh=True)), n_maps)


def step_baseline(n_maps):
    return _rates(dict(no_save={}, device=dict(save=True, device_output=True)), n_maps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--maps", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3, help="--baseline-tree: timed runs per case and tree, alternating between the trees")
    ap.add_argument("--skip-tester", action="store_true")
    ap.add_argument("--skip-sizes", action="store_true")
    ap.add_argument("--baseline-tree", default=None, help="a built checkout to compare Tester.run without the new flag with")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bokeh_export.json"))
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.baseline_tree) if a.step == "baseline_other" else ROOT)
        EB.begin_step()
        if a.step in SIZES:
            res = step_size(a.step, a.reps)
        elif a.step == "tester":
            res = step_tester(a.maps)
        else:
            res = step_baseline(a.maps)
        return EB.end_step(res)
    steps = [s for s in STEPS if not s.startswith("baseline") and not (a.skip_tester and s == "tester") and not (a.skip_sizes and s in SIZES)]
    args = ["--reps", a.reps, "--maps", a.maps] + (["--baseline-tree", a.baseline_tree] if a.baseline_tree else [])
    out = EB.run_steps(__file__, steps, a.step_timeout, args)
    if a.baseline_tree:
        runs = [EB.run_steps(__file__, ["baseline", "baseline_other"], a.step_timeout, args) for _ in range(a.runs)]
        cases = [c for c in runs[0]["baseline"] if c in ("no_save", "device")]
        out["baseline"] = {tree: {**{c: v for c, v in runs[0][key].items() if c not in cases}, **{c: [r[key][c] for r in runs] for c in cases}}
                           for tree, key in (("this_tree", "baseline"), ("other_tree", "baseline_other"))}
    return EB.report(out, a.out)


if __name__ == "__main__":
    sys.exit(main())
