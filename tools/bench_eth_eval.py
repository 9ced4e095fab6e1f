#!/usr/bin/env python
"""Cost of the ETH3D dataset evaluation (datasets.ETHDataset): one JSON line (also written to ``--out``, default profiles/eth_eval.json).

  python tools/bench_eth_eval.py [--reps 20] [--maps 4] [--skip-tester] [--out PATH]

Every GPU step runs in a child process of its own under a time limit (``--step-timeout`` seconds); the first step that does not
exit with status 0 ends the run (nothing more is started on the GPU) and the tool exits with that status.

Sizes are ETH3D's: a 24 MP photograph (4000 x 6000) resized to 2160 x 3840, ground truth 4032 x 6048, prediction 2160 x 3840.
- step ``image``: the image stage per frame.
    ``new_ms``     H2D of the photograph's BYTES from pinned memory + ops.u8_image_resize;
    ``parent_ms``  the reference's lines on the host (eth_dataset.py:150-161: / 255, F.interpolate bilinear align_corners=True on torch's
                   CPU) + H2D of the resized float image.
- step ``metrics``: ETHDataset.get_metrics per frame.
    ``new_ms``     ops.image_edge_region + ONE fused scoring pass over the three pixel sets, the prediction's resize inside it;
    ``parent_ms``  what the parent commit allows: eth_dataset.py:261-272 as torch ops on the device (float maps at ground-truth size)
                   and three metrics.compute_metrics_device calls (mask / ~mask / none).
  Wall-clock medians of ``--reps`` calls (parent: of 3) with a device synchronisation at each end, after a warm-up; ``*_alloc_bytes``:
  device bytes ALLOCATED per frame, from the caching allocator's counter (``allocated_bytes.all.allocated``) around one call.
- step ``tester``: Tester.run maps/s on v2_zoe_4k_r32 (synthetic weights, f16f6) over a synthetic ETH3D tree (JPEG photographs, raw
  float32 ground truth), with ground truth and with it dropped from the items.
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import evalbench as EB  # noqa: E402
from evalbench import alloc_bytes, wall_ms  # noqa: E402
MIN_DEPTH, MAX_DEPTH = 1e-3, 80
PHOTO, RAW, GT = (4000, 6000), (2160, 3840), (4032, 6048)
STEPS = ("image", "metrics", "tester")


def photograph(shape, k=0):
    """uint8 [h, w, 3]: smooth shading, two objects with sharp outlines and fine texture"""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 90 + 50 * np.sin(x / (211.0 + k)) * np.cos(y / 173.0) + 8 * np.sin(x / 3.0) * np.sin(y / 5.0)
    base += 70 * (x > (0.55 + 0.02 * k) * w) * (y > 0.3 * h) - 45 * (np.hypot(x - 0.25 * w, y - 0.5 * h) < 0.18 * h)
    img = np.stack([base, base * 0.9 + 10, base * 0.8 + 25], axis=-1)
    return np.clip(img, 0, 255).astype(np.uint8)


def depth_map(shape, k=0):
    """metric depth with planes, a disc, fine texture and holes (inf / NaN), float32"""
    h, w = shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    d = 3.0 + 6.0 * (x > (0.55 + 0.02 * k) * w) + 2.5 * (np.hypot(x - 0.25 * w, y - 0.5 * h) < 0.18 * h) + 0.2 * np.sin(y / 37.0) * np.cos(x / 53.0)
    d = d.astype(np.float32)
    d[::97, ::89] = np.inf
    d[5::211, 7::193] = np.nan
    return d


def step_image(reps):
    from patchrefinerv2_amd import ops
    px = photograph(PHOTO)
    pin = torch.from_numpy(px).pin_memory()

    def new():
        return ops.u8_image_resize(pin.cuda(non_blocking=True), *RAW)

    def parent():  # eth_dataset.py:150-161, then the float image to the device
        image = px.astype(np.float32) / 255.0
        t = F.interpolate(torch.from_numpy(image).unsqueeze(0).permute(0, 3, 1, 2), RAW, mode="bilinear", align_corners=True)
        return t[0].contiguous().cuda()
    diff = float((new() - parent()).abs().max())
    return dict(photo=list(PHOTO), out=list(RAW), new_ms=wall_ms(new, reps), parent_ms=wall_ms(parent, 3, warm=1),
                new_alloc_bytes=alloc_bytes(new), parent_alloc_bytes=alloc_bytes(parent), h2d_bytes=dict(new=px.size, parent=3 * RAW[0] * RAW[1] * 4),
                max_abs_diff_new_vs_parent=float(f"{diff:.3e}"))


def edge_area_torch(image, shape, frac=0.5):
    """eth_dataset.py:261-272 as torch ops on the image's device (kornia's Sobel / 8 with replicate padding and its 3 x 3 reflect blur
    written as shifted sums) -> bool [1, 1, H, W]"""
    p = F.pad(image[None], (1, 1, 1, 1), mode="replicate")[0]
    u, c, d = p[:, :-2], p[:, 1:-1], p[:, 2:]
    gx = ((u[:, :, 2:] - u[:, :, :-2]) + 2 * (c[:, :, 2:] - c[:, :, :-2]) + (d[:, :, 2:] - d[:, :, :-2])) / 8
    gy = ((d[:, :, :-2] - u[:, :, :-2]) + 2 * (d[:, :, 1:-1] - u[:, :, 1:-1]) + (d[:, :, 2:] - u[:, :, 2:])) / 8
    g = ((gx ** 2 + gy ** 2) ** (1 / 2)).sum(dim=0, keepdim=True)[None]
    edge = g.ge(g.max() * frac).float()
    k = torch.exp(-(torch.arange(3, dtype=torch.float32, device=image.device) - 1) ** 2 / 18.0)
    k = k / k.sum()
    q = F.pad(edge, (1, 1, 0, 0), mode="reflect")
    edge = k[0] * q[..., :-2] + k[1] * q[..., 1:-1] + k[2] * q[..., 2:]
    q = F.pad(edge, (0, 0, 1, 1), mode="reflect")
    edge = k[0] * q[..., :-2, :] + k[1] * q[..., 1:-1, :] + k[2] * q[..., 2:, :]
    return F.interpolate(edge, size=tuple(shape), mode="bilinear", align_corners=True) > 0


def step_metrics(reps):
    from patchrefinerv2_amd import metrics as M, ops
    from patchrefinerv2_amd.tester import ETHDataset
    image = ops.u8_image_resize(torch.from_numpy(photograph(PHOTO)).cuda(), *RAW)
    depth, boundary = ops.gt_decode(torch.from_numpy(depth_map(GT)).cuda(), "eth3d", th=1.0)
    gt = depth[None, None]
    lo = F.interpolate(gt, RAW, mode="bilinear", align_corners=False)
    pred = (lo.clamp(min=0.5) * (1 + 0.05 * torch.sin(torch.arange(RAW[1], device="cuda") / 11.0))).contiguous()
    ds = ETHDataset.__new__(ETHDataset)
    ds.min_depth, ds.max_depth = MIN_DEPTH, MAX_DEPTH
    kw = dict(disp_gt_edges=boundary, min_depth_eval=MIN_DEPTH, max_depth_eval=MAX_DEPTH, garg_crop=False, eigen_crop=False, dataset="")

    def new():
        return ds.get_metrics(gt, pred, disp_gt_edges=boundary, image_hr=image)

    def new_region():
        return ops.image_edge_region(image, *GT)

    def parent_region():
        return edge_area_torch(image, GT)

    def parent():
        mask = parent_region()
        out = {}
        for pre, m in (("edge_", mask), ("noedge_", torch.logical_not(mask)), ("", None)):
            out.update({pre + k: v for k, v in M.compute_metrics_device(gt, pred, additional_mask=m, **kw).items()})
        return out
    a, b = new(), parent()
    agree = max(abs(a[k] - b[k]) / max(1e-12, abs(b[k])) for k in b if not (np.isnan(a[k]) and np.isnan(b[k])))
    mask_diff = int((new_region().bool() != parent_region()[0, 0]).sum())
    return dict(image=list(RAW), gt=list(GT), pred=list(RAW), edge_share=round(float(new_region().float().mean()), 5),
                new_ms=dict(edge_region=wall_ms(new_region, reps), get_metrics=wall_ms(new, reps)),
                parent_ms=dict(edge_region=wall_ms(parent_region, 3, warm=1), get_metrics=wall_ms(parent, 3, warm=1)),
                new_alloc_bytes=dict(edge_region=alloc_bytes(new_region), get_metrics=alloc_bytes(new)),
                parent_alloc_bytes=dict(edge_region=alloc_bytes(parent_region), get_metrics=alloc_bytes(parent)),
                mask_pixels_differing=mask_diff, max_rel_diff_new_vs_parent=float(f"{agree:.3e}"))


def step_tester(n_maps):
    from PIL import Image
    from patchrefinerv2_amd.tester import ETHDataset
    w, model = EB.workload_model()
    with tempfile.TemporaryDirectory() as root:
        lines = []
        for k in range(n_maps):
            img, gt = os.path.join(root, f"DSC_{k:04d}.JPG"), os.path.join(root, f"DSC_{k:04d}.depth")
            Image.fromarray(photograph(PHOTO, k)).save(img, quality=92)
            depth_map(GT, k).tofile(gt)
            lines.append(f"{img} {gt}\n")
        split = os.path.join(root, "split.txt")
        with open(split, "w") as f:
            f.writelines(lines)
        ds = ETHDataset("infer", split, dict(input_size_deep=[384, 512], input_size_shallow=list(w["raw"])), MIN_DEPTH, MAX_DEPTH, gt_shape=GT)
        out, keys = EB.gt_pair_maps_s(model, ds, w, n_maps)
        ds.close()
    return dict(workload=EB.WORKLOAD, maps=n_maps, photo=list(PHOTO), gt=list(GT), metric_keys=keys, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--maps", type=int, default=4)
    ap.add_argument("--skip-tester", action="store_true")
    EB.add_step_arguments(ap, STEPS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eth_eval.json"))
    a = ap.parse_args()
    if a.step:
        EB.begin_step()
        return EB.end_step(step_tester(a.maps) if a.step == "tester" else (step_image if a.step == "image" else step_metrics)(a.reps))
    out = EB.run_steps(__file__, STEPS[:2] if a.skip_tester else STEPS, a.step_timeout, ["--reps", a.reps, "--maps", a.maps])
    return EB.report(out, a.out)


if __name__ == "__main__":
    sys.exit(main())
