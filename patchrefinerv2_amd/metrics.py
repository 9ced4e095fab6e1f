"""Depth-evaluation metrics and colour maps of the reference's Tester (host side, numpy).

compute_errors      estimator/utils/metric.py:11-50   (delta1-3, AbsRel, RMSE, log10, RMSE-log, SILog, SqRel)
soft_edge_error     estimator/utils/metric.py:53-72   (min |gt shifted - pred| over a (2r+1)^2 window)
get_boundaries      estimator/utils/metric.py:74-85   (disparity jumps > th; dilation needs cv2 -> dilation=0 only)
compute_metrics     estimator/utils/metric.py:87-149  (resize, clamp, valid / crop masks, optional SEE on gt edges)
colorize            estimator/utils/color.py:95-158   (percentile normalisation + matplotlib colour map, RGBA uint8)
compute_metrics_fused  the same metrics from one fused GPU pass (csrc/evalgt.hip), optionally for three pixel sets at once and with the
                       resize of a low-resolution prediction inside that pass (fuse_resize)
compute_scale_and_shift   estimator/models/losses.py:523-544 (the least-squares scale and shift of a prediction inside a mask)
compute_ssi_metrics       estimator/models/losses.py:600-700 (ScaleAndShiftInvariantLoss' three modes as evaluation scores) and
                          compute_errors on the aligned prediction; float64 numpy, the oracle of compute_ssi_metrics_fused
                          (csrc/ssi_eval.hip: two fused GPU passes, one D2H); pinned by tests/golden/ssi_eval.npz
compute_boundary_f1       NOT in the reference: the scale-invariant boundary F1 of Depth Pro (Bochkovskii et al., 2024) from ratio tests on
                          neighbouring pixels, numpy; the specification and oracle of compute_boundary_f1_fused
                          (csrc/boundary_eval.hip: one fused GPU pass of integer counts, one D2H)
compute_uncertainty_metrics   NOT in the reference: the sparsification scores AUSE / AURG (Ilg et al. 2018; Poggi et al. 2020) of a
                          per-pixel uncertainty against ground truth, numpy; the specification and oracle of
                          compute_uncertainty_metrics_fused (csrc/sparsify.hip: thresholds by the radix select, one D2H)

Pinned by tests/golden/output_stage.npz (the reference functions imported by oracle/make_golden.py).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def compute_errors(gt: np.ndarray, pred: np.ndarray) -> dict:
    thresh = np.maximum(gt / pred, pred / gt)
    d = gt - pred
    err = np.log(pred) - np.log(gt)
    return dict(a1=(thresh < 1.25).mean(), a2=(thresh < 1.25 ** 2).mean(), a3=(thresh < 1.25 ** 3).mean(),
                abs_rel=np.mean(np.abs(d) / gt), rmse=np.sqrt((d ** 2).mean()),
                log_10=np.abs(np.log10(gt) - np.log10(pred)).mean(),
                rmse_log=np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean()),
                silog=np.sqrt(np.mean(err ** 2) - np.mean(err) ** 2) * 100, sq_rel=np.mean(d ** 2 / gt))


def _shift(data: np.ndarray, dx: int, dy: int, fill=0) -> np.ndarray:
    out = np.roll(data, dx, axis=1)
    if dx < 0:
        out[:, dx:] = fill
    elif dx > 0:
        out[:, :dx] = fill
    out = np.roll(out, dy, axis=0)
    if dy < 0:
        out[dy:, :] = fill
    elif dy > 0:
        out[:dy, :] = fill
    return out


def soft_edge_error(pred: np.ndarray, gt: np.ndarray, radius: int = 1) -> np.ndarray:
    diffs = [np.abs(_shift(gt, i, j, 0) - pred) for i in range(-radius, radius + 1) for j in range(-radius, radius + 1)]
    return np.minimum.reduce(diffs)


def get_boundaries(disp: np.ndarray, th: float = 1.0, dilation: int = 0) -> np.ndarray:
    if dilation > 0:
        raise NotImplementedError("get_boundaries(dilation > 0) uses cv2.dilate (un-vendored); every dataset branch of the "
                                  "reference calls it with dilation=0 (general_dataset.py:88-143)")
    dy = np.abs(disp[1:, :] - disp[:-1, :]) > th
    dx = np.abs(disp[:, 1:] - disp[:, :-1]) > th
    ey = np.logical_or(np.pad(dy, ((1, 0), (0, 0))), np.pad(dy, ((0, 1), (0, 0))))
    ex = np.logical_or(np.pad(dx, ((0, 0), (1, 0))), np.pad(dx, ((0, 0), (0, 1))))
    return np.logical_or(ey, ex).astype(np.float32)


def compute_metrics(gt, pred, interpolate=True, garg_crop=False, eigen_crop=True, dataset="nyu", min_depth_eval=0.1,
                    max_depth_eval=10, disp_gt_edges=None, additional_mask=None) -> dict:
    if gt.shape[-2:] != pred.shape[-2:] and interpolate:
        pred = F.interpolate(pred, gt.shape[-2:], mode="bilinear", align_corners=False).squeeze()
    pred = pred.squeeze().cpu().numpy().copy()
    pred[pred < min_depth_eval] = min_depth_eval
    pred[pred > max_depth_eval] = max_depth_eval
    pred[np.isinf(pred)] = max_depth_eval
    pred[np.isnan(pred)] = min_depth_eval
    gt_depth = gt.squeeze().cpu().numpy()
    valid = np.logical_and(gt_depth > min_depth_eval, gt_depth < max_depth_eval)
    eval_mask = np.ones(valid.shape)
    if garg_crop or eigen_crop:
        h, w = gt_depth.shape
        eval_mask = np.zeros(valid.shape)
        if garg_crop:
            eval_mask[int(0.40810811 * h):int(0.99189189 * h), int(0.03594771 * w):int(0.96405229 * w)] = 1
        elif dataset == "kitti":
            eval_mask[int(0.3324324 * h):int(0.91351351 * h), int(0.0359477 * w):int(0.96405229 * w)] = 1
        else:
            eval_mask[45:471, 41:601] = 1
    valid = np.logical_and(valid, eval_mask)
    if additional_mask is not None:
        valid = np.logical_and(valid, additional_mask.squeeze().detach().cpu().numpy())
    metrics = compute_errors(gt_depth[valid], pred[valid])
    if disp_gt_edges is not None:
        edges = disp_gt_edges.squeeze().numpy() if isinstance(disp_gt_edges, torch.Tensor) else np.squeeze(disp_gt_edges)
        mask = np.logical_and(valid.squeeze(), edges)
        see = torch.tensor([0])
        if mask.sum() > 0:
            see = soft_edge_error(pred, gt_depth)[mask].mean()
        metrics["see"] = see
    return metrics


@torch.no_grad()
def compute_metrics_device(gt: torch.Tensor, pred: torch.Tensor, interpolate=True, garg_crop=False, eigen_crop=True, dataset="nyu",
                           min_depth_eval=0.1, max_depth_eval=10, disp_gt_edges=None, additional_mask=None) -> dict:
    """``compute_metrics`` (estimator/utils/metric.py:87-149) on the tensors' device -- the prediction does not have to leave the
    GPU to be scored: same clamping, masks, error formulas and soft-edge error; the reductions accumulate in
    float64 (the numpy version sums float32 pairwise: agreement to ~1e-6 relative, tests/test_host_logic.py)."""
    dev = pred.device
    gt = gt.to(dev)
    if gt.shape[-2:] != pred.shape[-2:] and interpolate:
        pred = F.interpolate(pred, gt.shape[-2:], mode="bilinear", align_corners=False)
    p = pred.squeeze().float().clone()
    p = torch.where(torch.isnan(p), torch.full_like(p, min_depth_eval), p)  # (order as the reference: < min, > max, inf, nan)
    p = p.clamp(min_depth_eval, max_depth_eval)
    g = gt.squeeze().float()
    valid = (g > min_depth_eval) & (g < max_depth_eval)
    if garg_crop or eigen_crop:
        y0, y1, x0, x1 = _eval_crop(*g.shape, garg_crop, eigen_crop, dataset)
        m = torch.zeros_like(valid)
        m[y0:y1, x0:x1] = True
        valid &= m
    if additional_mask is not None:
        valid &= additional_mask.squeeze().to(dev).bool()
    gv, pv = g[valid].double(), p[valid].double()
    thresh = torch.maximum(gv / pv, pv / gv)
    d = gv - pv
    err = torch.log(pv) - torch.log(gv)
    out = dict(a1=(thresh < 1.25).double().mean(), a2=(thresh < 1.25 ** 2).double().mean(), a3=(thresh < 1.25 ** 3).double().mean(),
               abs_rel=(d.abs() / gv).mean(), rmse=(d ** 2).mean().sqrt(), log_10=(torch.log10(gv) - torch.log10(pv)).abs().mean(),
               rmse_log=(err ** 2).mean().sqrt(), silog=((err ** 2).mean() - err.mean() ** 2).sqrt() * 100, sq_rel=(d ** 2 / gv).mean())
    if disp_gt_edges is not None:
        edges = torch.as_tensor(disp_gt_edges).squeeze().to(dev) != 0
        mask = valid & edges
        see = torch.zeros((), device=dev, dtype=torch.float64)
        if bool(mask.any()):
            best = None
            for i in (-1, 0, 1):      # soft_edge_error(radius=1): min over the 3 x 3 shifts of gt (zero-filled borders)
                for j in (-1, 0, 1):
                    sh = torch.zeros_like(g)
                    ys, yd = (slice(0, g.shape[0] - j), slice(j, None)) if j >= 0 else (slice(-j, None), slice(0, g.shape[0] + j))
                    xs, xd = (slice(0, g.shape[1] - i), slice(i, None)) if i >= 0 else (slice(-i, None), slice(0, g.shape[1] + i))
                    sh[yd, xd] = g[ys, xs]
                    diff = (sh - p).abs()
                    best = diff if best is None else torch.minimum(best, diff)
            see = best[mask].double().mean()
        out["see"] = see
    keys = list(out)
    vals = torch.stack([out[k].double() for k in keys]).cpu().tolist()  # one D2H of ten scalars
    return dict(zip(keys, vals))


def _eval_crop(h, w, garg_crop, eigen_crop, dataset):
    """the rows / columns compute_metrics keeps (metric.py:108-120) as (y0, y1, x0, x1), clipped to the frame like numpy's slices"""
    if not (garg_crop or eigen_crop):
        return 0, h, 0, w
    if garg_crop:
        y0, y1, x0, x1 = int(0.40810811 * h), int(0.99189189 * h), int(0.03594771 * w), int(0.96405229 * w)
    elif dataset == "kitti":
        y0, y1, x0, x1 = int(0.3324324 * h), int(0.91351351 * h), int(0.0359477 * w), int(0.96405229 * w)
    else:
        y0, y1, x0, x1 = 45, 471, 41, 601
    y0, y1, x0, x1 = min(y0, h), min(y1, h), min(x0, w), min(x1, w)
    return y0, max(y0, y1), x0, max(x0, x1)


def metrics_from_sums(s, with_see: bool) -> dict:
    """one pixel set's twelve sums (ops.depth_metrics) -> the dict of compute_errors (+ ``see``): means over the valid count, NaN when
    it is zero (numpy's mean of an empty array); silog from the sums of err^2 and err; see 0 without a valid boundary pixel"""
    n, c1, c2, c3, abs_rel, d2, l10, e2, e1, sq_rel, n_see, see = (float(v) for v in s)
    nan = float("nan")

    def mean(v):
        return v / n if n else nan
    var = mean(e2) - mean(e1) ** 2 if n else nan
    out = dict(a1=mean(c1), a2=mean(c2), a3=mean(c3), abs_rel=mean(abs_rel), rmse=float(np.sqrt(mean(d2))), log_10=mean(l10),
               rmse_log=float(np.sqrt(mean(e2))), silog=float(np.sqrt(var)) * 100 if not var < 0 else nan, sq_rel=mean(sq_rel))
    if with_see:
        out["see"] = see / n_see if n_see else 0.0
    return out


def _fused_inputs(gt, pred, interpolate, fuse_resize, garg_crop, eigen_crop, dataset):
    """the opening of the fused scoring calls -> (g [B, H, W], p, single, lowres, crop): both maps as fp32 frames on the GPU (the
    prediction's device, else the ground truth's, else 'cuda'); ``lowres``: a prediction of another shape stays as it is (the kernel
    samples it), otherwise F.interpolate resizes it first"""
    dev = pred.device if pred.is_cuda else (gt.device if gt.is_cuda else torch.device("cuda"))
    gt, pred = gt.to(dev), pred.to(dev)
    lowres = bool(fuse_resize) and interpolate and gt.shape[-2:] != pred.shape[-2:]
    if gt.shape[-2:] != pred.shape[-2:] and interpolate and not lowres:
        p4 = pred if pred.dim() == 4 else pred.reshape(-1, 1, *pred.shape[-2:])
        pred = F.interpolate(p4.float(), gt.shape[-2:], mode="bilinear", align_corners=False)
    g, single = _frames_of(gt.float())
    p = pred.float().reshape(g.shape[0], *pred.shape[-2:]) if lowres else pred.float().reshape(g.shape)
    return g, p, single, lowres, _eval_crop(g.shape[1], g.shape[2], garg_crop, eigen_crop, dataset)


@torch.no_grad()
def compute_metrics_fused(gt: torch.Tensor, pred: torch.Tensor, interpolate=True, garg_crop=False, eigen_crop=True, dataset="nyu",
                          min_depth_eval=0.1, max_depth_eval=10, disp_gt_edges=None, additional_mask=None, region=None, fuse_resize=False):
    """``compute_metrics`` (estimator/utils/metric.py:87-149) from one fused pass on the GPU (csrc/evalgt.hip, ops.depth_metrics): the
    same clamping, masks, crops, error formulas and soft-edge error as ``compute_metrics_device``, as twelve float64 sums per frame
    and ONE D2H of them per call.  ``region`` (a mask) adds ``edge_*`` (inside it) and ``noedge_*`` (outside it) copies of every key
    from the same read -- the three scoring calls of datasets.ImageDataset._edge_metrics in one.  ``additional_mask`` scores inside
    that mask only, as in compute_metrics.  A dict for one map ([H, W] / [1, 1, H, W]), a list of dicts for B maps.  Inputs that
    are on the host are copied to the GPU: there is no CPU path.  ``fuse_resize``: a prediction of another resolution is sampled inside
    the scoring kernel (ops.depth_metrics_lowres: the operations of F.interpolate, without writing the resized map) instead of being
    resized first; the default keeps the resize."""
    from . import ops
    if additional_mask is not None and region is not None:
        raise ValueError("compute_metrics_fused: give additional_mask or region, not both")
    g, p, single, lowres, crop = _fused_inputs(gt, pred, interpolate, fuse_resize, garg_crop, eigen_crop, dataset)

    def mask(m):
        return None if m is None else torch.as_tensor(m).to(g.device).reshape(g.shape)
    inside = region if region is not None else additional_mask
    score = ops.depth_metrics_lowres if lowres else ops.depth_metrics
    sums = score(g, p, mask(disp_gt_edges), mask(inside), min_depth_eval, max_depth_eval, crop).cpu().numpy()  # the one D2H
    see = disp_gt_edges is not None
    rows = []
    for f in range(g.shape[0]):
        if additional_mask is not None:
            out = metrics_from_sums(sums[f, 1], see)
        else:
            out = metrics_from_sums(sums[f, 0], see)
            if region is not None:
                for name, k in (("edge", 1), ("noedge", 2)):
                    out.update({f"{name}_{key}": v for key, v in metrics_from_sums(sums[f, k], see).items()})
        rows.append(out)
    return rows[0] if single else rows


# ------------------------------------------------------------------------------------------------------------------
# Scale-and-shift-invariant evaluation: how good a prediction's structure is once its global scale and offset are taken out.
#   compute_scale_and_shift        estimator/models/losses.py:523-544
#   ScaleAndShiftInvariantLoss     estimator/models/losses.py:600-700 (ssi L1; ssi / plain gradient matching; the 'inverse' fit)
# The mask is compute_metrics' (valid range and crop); the prediction is not clamped (the loss does not clamp it); every score divides
# by the mask count N, not by the number of pairs; N <= 1 gives NaN everywhere (the loss' ``prediction * 0.0`` there is a training
# guard).  A pixel outside the mask is never looked at (the reference multiplies by the mask, which lets a NaN there through).
# Pinned by tests/golden/ssi_eval.npz (tools/make_ssi_golden.py runs the reference's own functions in float64).
# ------------------------------------------------------------------------------------------------------------------
SSI_ERROR_KEYS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel")
SSI_KEYS = ("ssi_scale", "ssi_shift", "ssi_l1", "ssi_gm", "gm", "ssi_gm_inv") + tuple("ssi_" + k for k in SSI_ERROR_KEYS)


def _np64(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def compute_scale_and_shift(pred, gt, mask):
    """losses.py:523-544 in float64: the (scale, shift) that minimise sum mask (scale * pred + shift - gt)^2 from the 2 x 2 normal
    equations, both 0 when the determinant is not positive.  [H, W] maps -> two floats; [B, H, W] -> two arrays [B]."""
    m = np.asarray(mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else mask).astype(bool)
    p, g = np.where(m, _np64(pred), 0.0), np.where(m, _np64(gt), 0.0)
    ax = (-2, -1)
    a00, a01, a11 = (p * p).sum(ax), p.sum(ax), m.sum(ax).astype(np.float64)
    b0, b1 = (p * g).sum(ax), g.sum(ax)
    det = a00 * a11 - a01 * a01
    ok = det > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        x0 = np.where(ok, (a11 * b0 - a01 * b1) / det, 0.0)
        x1 = np.where(ok, (-a01 * b0 + a00 * b1) / det, 0.0)
    return (float(x0), float(x1)) if x0.ndim == 0 else (x0, x1)


def _ssi_scores(p, g, m) -> dict:
    """one frame: float64 maps p, g and the bool mask m -> scale, shift and the four scores"""
    n = float(m.sum())
    p, g = np.where(m, p, 0.0), np.where(m, g, 0.0)  # (outside the mask nothing is looked at)
    vm, hm = m[:-2] & m[2:], m[:, :-2] & m[:, 2:]
    s, t = compute_scale_and_shift(p, g, m)

    def gm(d):  # losses.py:683-696: sum(h) + sum(v) over the pairs inside the mask
        return float(np.abs(d[:, :-2] - d[:, 2:])[hm].sum() + np.abs(d[:-2] - d[2:])[vm].sum())
    vp, vg, hp, hg = p[:-2] - p[2:], g[:-2] - g[2:], p[:, :-2] - p[:, 2:], g[:, :-2] - g[:, 2:]
    sv, tv = compute_scale_and_shift(vp, vg, vm)
    sh, th = compute_scale_and_shift(hp, hg, hm)
    inv = float(np.abs(sv * vp + tv - vg)[vm].sum() + np.abs(sh * hp + th - hg)[hm].sum())  # :641-644
    with np.errstate(divide="ignore", invalid="ignore"):
        return dict(ssi_scale=s, ssi_shift=t, ssi_l1=float(np.abs(s * p + t - g)[m].sum()) / n, ssi_gm=gm((s * p + t - g) * m) / n,
                    gm=gm((p - g) * m) / n, ssi_gm_inv=inv / n)


def compute_ssi_metrics(gt, pred, interpolate=True, garg_crop=False, eigen_crop=True, dataset="nyu", min_depth_eval=0.1, max_depth_eval=10):
    """The scale-and-shift-invariant scores of one frame on the host, float64 from the fp32 maps: ``ssi_scale`` / ``ssi_shift``
    (compute_scale_and_shift inside compute_metrics' mask), ``ssi_l1``, ``ssi_gm``, ``gm`` and ``ssi_gm_inv``
    (ScaleAndShiftInvariantLoss with ssi / ssi + grad_matching / grad_matching alone / inverse), and ``ssi_a1 ... ssi_sq_rel``:
    compute_metrics of the aligned prediction (scale * pred + shift rounded once to fp32), the fp32 values widened to float64 so that
    its sums are float64 too.  A prediction of another shape is resized as compute_metrics resizes it (bilinear, align_corners=False)."""
    gt, pred = torch.as_tensor(gt).detach().cpu().float(), torch.as_tensor(pred).detach().cpu().float()
    if gt.shape[-2:] != pred.shape[-2:] and interpolate:
        pred = F.interpolate(pred.reshape(1, 1, *pred.shape[-2:]), gt.shape[-2:], mode="bilinear", align_corners=False)
    g32 = gt.reshape(gt.shape[-2:]).numpy()
    p32 = pred.reshape(pred.shape[-2:]).numpy()
    h, w = g32.shape
    y0, y1, x0, x1 = _eval_crop(h, w, garg_crop, eigen_crop, dataset)
    m = np.zeros((h, w), bool)
    m[y0:y1, x0:x1] = True
    with np.errstate(invalid="ignore"):
        m &= (g32 > np.float32(min_depth_eval)) & (g32 < np.float32(max_depth_eval))  # fp32 comparisons; a NaN is not valid
    if m.sum() <= 1:
        return {k: float("nan") for k in SSI_KEYS}
    p, g = p32.astype(np.float64), g32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out = _ssi_scores(p, g, m)
        aligned = (out["ssi_scale"] * p + out["ssi_shift"]).astype(np.float32)
    # (the bounds as the fp32 values an fp32 map is compared with and clamped to: float64 arithmetic, fp32 decisions)
    errs = compute_metrics(torch.from_numpy(np.where(m, g, 0.0)), torch.from_numpy(aligned.astype(np.float64)), interpolate=False,
                           garg_crop=garg_crop, eigen_crop=eigen_crop, dataset=dataset, min_depth_eval=float(np.float32(min_depth_eval)),
                           max_depth_eval=float(np.float32(max_depth_eval)))
    out.update({"ssi_" + k: float(errs[k]) for k in SSI_ERROR_KEYS})
    return out


def ssi_from_values(v) -> dict:
    """one frame's row of ops.ssi_metrics (include/prv2.h prv2_ssi_metrics) -> the dict of compute_ssi_metrics"""
    v = [float(x) for x in v]
    n = v[6]
    if n <= 1:
        return {k: float("nan") for k in SSI_KEYS}
    out = dict(ssi_scale=v[0], ssi_shift=v[1], ssi_l1=v[22] / n, ssi_gm=(v[24] + v[23]) / n, gm=(v[26] + v[25]) / n,
               ssi_gm_inv=(v[27] + v[28]) / n)
    out.update({"ssi_" + k: x for k, x in metrics_from_sums(v[29:41], False).items()})
    return out


@torch.no_grad()
def compute_ssi_metrics_fused(gt: torch.Tensor, pred: torch.Tensor, interpolate=True, garg_crop=False, eigen_crop=True, dataset="nyu",
                              min_depth_eval=0.1, max_depth_eval=10, fuse_resize=False):
    """``compute_ssi_metrics`` from two fused passes on the GPU (csrc/ssi_eval.hip, ops.ssi_metrics): the fits are solved on the device
    between the passes, ONE D2H of 41 float64 values per frame.  A dict for one map ([H, W] / [1, 1, H, W]), a list of dicts for B
    maps.  Inputs on the host are copied to the GPU.  ``fuse_resize``: a prediction of another resolution is sampled inside the kernels
    (the operations of F.interpolate, the resized map is never written) instead of being resized first."""
    from . import ops
    g, p, single, _lowres, crop = _fused_inputs(gt, pred, interpolate, fuse_resize, garg_crop, eigen_crop, dataset)
    vals = ops.ssi_metrics(g, p, min_depth_eval, max_depth_eval, crop).cpu().numpy()  # the one D2H
    rows = [ssi_from_values(v) for v in vals]
    return rows[0] if single else rows


# ------------------------------------------------------------------------------------------------------------------
# Scale-invariant boundary F1 (Depth Pro, Bochkovskii et al., 2024): how sharp a prediction's occluding boundaries are, and whether
# the depth step across them has the right size and direction.  NOT in the reference; this is the definition (include/prv2.h
# "Boundary F1 evaluation" states it for the kernel), compute_boundary_f1 is its numpy statement and the oracle of
# compute_boundary_f1_fused (csrc/boundary_eval.hip).
#   Inputs       ground truth g [H, W] fp32; prediction p brought to [H, W] exactly as compute_metrics brings it there
#                (F.interpolate(bilinear, align_corners=False), or the in-kernel sample); min_depth_eval, max_depth_eval; the crop window
#                of _eval_crop.
#   Mask         A pixel is valid when it lies inside the crop and g > min && g < max.  A NaN ground truth is not valid.
#   Prediction cleaning   The prediction at a valid pixel is cleaned as compute_metrics cleans it: NaN -> min, clamp to [min, max].
#                Every compared value is therefore finite and positive.  The prediction is never read at an invalid pixel.
#   Pairs        A horizontal pair is (x, y), (x + 1, y) and a vertical pair is (x, y), (x, y + 1).  A pair counts only if BOTH pixels
#                are valid.  n_h and n_v are the numbers of such pairs.
#   Thresholds   t_i = float32(np.linspace(1.05, 1.25, T)[i]), with T = 10 by default and 1 <= T <= 16.
#   Boundary test   All tests are fp32 compare-after-multiply with no division: a > t * b, product rounded to fp32, not contracted.
#                For a depth map d, a pair (a, b) (a = left or top value, b = right or bottom value) and a threshold t:
#                horizontal  L: a > t * b (left is farther); R: b > t * a;   vertical  T: a > t * b (top is farther); B: b > t * a.
#   Relation to Depth Pro   Depth Pro applies the ratio test to inverse depth.  That swaps L <-> R and T <-> B in prediction and ground
#                truth alike, so the counts below are the same up to the rounding of the division.
#   Counts       Per threshold i and direction d in the order (L, T, R, B), over the valid pairs: tp[i][d] = pairs flagged in
#                prediction AND ground truth; np[i][d] = flagged in the prediction; ng[i][d] = flagged in the ground truth.
#   Per-threshold scores   P_i = 1/4 sum_d tp / max(np, 1);  R_i = 1/4 sum_d tp / max(ng, 1);
#                F_i = 0 if P_i + R_i == 0 else 2 P_i R_i / (P_i + R_i).
#   Weights      w_i = t_i / sum t, computed in float64 from the fp32 thresholds.
#   Keys         si_boundary_f1 = sum w_i F_i, si_boundary_p = sum w_i P_i, si_boundary_r = sum w_i R_i.  n_h + n_v == 0 gives NaN for
#                all three: nothing can be scored then, and the frame drops out of the dataset's nanmean.  curves=True adds
#                boundary_thresholds, boundary_p, boundary_r, boundary_f1 (lists of length T).
# ------------------------------------------------------------------------------------------------------------------
BOUNDARY_KEYS = ("si_boundary_f1", "si_boundary_p", "si_boundary_r")
BOUNDARY_MAX_THRESHOLDS = 16  # PRV2_BOUNDARY_MAX_THRESHOLDS


def boundary_thresholds(T: int = 10) -> np.ndarray:
    """the T ratios float32(np.linspace(1.05, 1.25, T)), 1 <= T <= 16"""
    if not 1 <= int(T) <= BOUNDARY_MAX_THRESHOLDS:
        raise ValueError(f"boundary_thresholds: T = {T} is not in [1, {BOUNDARY_MAX_THRESHOLDS}]")
    return np.linspace(1.05, 1.25, int(T)).astype(np.float32)


def _boundary_thresholds(thresholds) -> np.ndarray:
    """``thresholds`` (None: the ten defaults) as a checked fp32 array: 1 .. 16 finite ratios > 1"""
    th = boundary_thresholds() if thresholds is None else np.asarray(thresholds, dtype=np.float32).reshape(-1)
    if not 1 <= th.size <= BOUNDARY_MAX_THRESHOLDS:
        raise ValueError(f"boundary F1: {th.size} thresholds, not in [1, {BOUNDARY_MAX_THRESHOLDS}]")
    if not (np.isfinite(th) & (th > 1)).all():
        raise ValueError(f"boundary F1: every threshold is a finite ratio > 1, got {th.tolist()}")
    return th


def boundary_counts(g32: np.ndarray, p32: np.ndarray, m: np.ndarray, thresholds) -> np.ndarray:
    """the row of ops.boundary_f1 for one frame, with whole-array boolean operations: fp32 ground truth and CLEANED fp32 prediction
    [H, W], the bool mask m and T thresholds -> float64 [2 + 12 T]: n_h, n_v, then for i, for d in (L, T, R, B): tp, np, ng"""
    th = np.asarray(thresholds, dtype=np.float32)
    g = np.where(m, g32, np.float32(1)).astype(np.float32)  # (outside the mask nothing is looked at)
    p = np.where(m, p32, np.float32(1)).astype(np.float32)
    hm, vm = m[:, :-1] & m[:, 1:], m[:-1] & m[1:]
    row = [float(hm.sum()), float(vm.sum())]

    def flags(d, t):  # L, T, R, B of one map: compare after the fp32 multiply
        ha, hb, va, vb = d[:, :-1], d[:, 1:], d[:-1], d[1:]
        return (ha > t * hb) & hm, (va > t * vb) & vm, (hb > t * ha) & hm, (vb > t * va) & vm
    with np.errstate(over="ignore"):
        for t in th:
            for fp, fg in zip(flags(p, t), flags(g, t)):
                row += [float((fp & fg).sum()), float(fp.sum()), float(fg.sum())]
    return np.asarray(row, dtype=np.float64)


def boundary_from_values(row, thresholds, curves=False) -> dict:
    """one frame's row of ops.boundary_f1 (include/prv2.h prv2_boundary_f1: n_h, n_v, then [T][L, T, R, B][tp, np, ng]) and its
    thresholds -> the dict of BOUNDARY_KEYS (``curves``: also boundary_thresholds / boundary_p / boundary_r / boundary_f1, lists of
    length T); NaN everywhere without a valid pair"""
    th = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    v = np.asarray(row, dtype=np.float64)
    if v.shape != (2 + 12 * th.size,):
        raise ValueError(f"boundary_from_values: a row of {v.size} values for {th.size} thresholds (2 + 12 T)")
    nan = float("nan")
    if v[0] + v[1] == 0:
        out = {k: nan for k in BOUNDARY_KEYS}
        if curves:
            out.update(boundary_thresholds=[float(t) for t in th], boundary_p=[nan] * th.size, boundary_r=[nan] * th.size,
                       boundary_f1=[nan] * th.size)
        return out
    c = v[2:].reshape(th.size, 4, 3)
    tp, n_p, n_g = c[..., 0], c[..., 1], c[..., 2]
    P = (tp / np.maximum(n_p, 1.0)).sum(1) / 4.0
    R = (tp / np.maximum(n_g, 1.0)).sum(1) / 4.0
    F1 = np.array([0.0 if a + b == 0 else 2.0 * a * b / (a + b) for a, b in zip(P, R)])
    w = th.astype(np.float64) / th.astype(np.float64).sum()
    out = dict(si_boundary_f1=float((w * F1).sum()), si_boundary_p=float((w * P).sum()), si_boundary_r=float((w * R).sum()))
    if curves:
        out.update(boundary_thresholds=[float(t) for t in th], boundary_p=P.tolist(), boundary_r=R.tolist(), boundary_f1=F1.tolist())
    return out


def compute_boundary_f1(gt, pred, interpolate=True, garg_crop=False, eigen_crop=True, dataset="nyu", min_depth_eval=0.1, max_depth_eval=10,
                        thresholds=None, curves=False, return_counts=False):
    """The scale-invariant boundary F1 of one frame on the host (the definition above): compute_metrics' own arguments, resize
    (bilinear, align_corners=False) and cleaning of the prediction, its mask (valid range and crop; a NaN ground truth is not valid), then
    the counts by whole-array boolean operations and the scores through ``boundary_from_values``.  Depth Pro applies the ratio test to
    inverse depth, which swaps L <-> R and T <-> B in prediction and ground truth alike: the same counts up to the rounding of its
    division.  ``return_counts``: (dict, the float64 row of ops.boundary_f1)."""
    th = _boundary_thresholds(thresholds)
    gt, pred = torch.as_tensor(gt).detach().cpu().float(), torch.as_tensor(pred).detach().cpu().float()
    if gt.shape[-2:] != pred.shape[-2:] and interpolate:
        pred = F.interpolate(pred.reshape(1, 1, *pred.shape[-2:]), gt.shape[-2:], mode="bilinear", align_corners=False)
    g32 = gt.reshape(gt.shape[-2:]).numpy()
    p32 = pred.reshape(pred.shape[-2:]).numpy().copy()
    mn, mx = np.float32(min_depth_eval), np.float32(max_depth_eval)
    with np.errstate(invalid="ignore"):
        p32[p32 < mn] = mn  # compute_metrics' cleaning (metric.py:98-101), the bounds as fp32 values
        p32[p32 > mx] = mx
        p32[np.isinf(p32)] = mx
        p32[np.isnan(p32)] = mn
        h, w = g32.shape
        y0, y1, x0, x1 = _eval_crop(h, w, garg_crop, eigen_crop, dataset)
        m = np.zeros((h, w), bool)
        m[y0:y1, x0:x1] = True
        m &= (g32 > mn) & (g32 < mx)  # fp32 comparisons; a NaN is not valid
    row = boundary_counts(g32, p32, m, th)
    out = boundary_from_values(row, th, curves)
    return (out, row) if return_counts else out


@torch.no_grad()
def compute_boundary_f1_fused(gt: torch.Tensor, pred: torch.Tensor, interpolate=True, garg_crop=False, eigen_crop=True, dataset="nyu",
                              min_depth_eval=0.1, max_depth_eval=10, thresholds=None, curves=False, fuse_resize=False):
    """``compute_boundary_f1`` from one fused pass on the GPU (csrc/boundary_eval.hip, ops.boundary_f1): the integer counts of every
    frame, ONE D2H of 2 + 12 T float64 values per frame, the scores through ``boundary_from_values`` (equal counts give equal floats).
    A dict for one map ([H, W] / [1, 1, H, W]), a list of dicts for B maps.  Inputs on the host are copied to the GPU: there is no CPU
    path.  ``fuse_resize``: a prediction of another resolution is sampled inside the kernel (the operations of F.interpolate, the
    resized map is never written) instead of being resized first."""
    from . import ops
    th = _boundary_thresholds(thresholds)
    g, p, single, _lowres, crop = _fused_inputs(gt, pred, interpolate, fuse_resize, garg_crop, eigen_crop, dataset)
    vals = ops.boundary_f1(g, p, min_depth_eval, max_depth_eval, crop, th).cpu().numpy()  # the one D2H
    rows = [boundary_from_values(v, th, curves) for v in vals]
    return rows[0] if single else rows


# ------------------------------------------------------------------------------------------------------------------
# Sparsification scores of a per-pixel uncertainty (the pseudo-label writer's ``uncertainty`` / ``count_map``): does a high uncertainty
# mark the pixels where the depth is wrong?  The definition (include/prv2.h "Sparsification" states it for the kernels):
#   valid   min < gt < max (compute_metrics' rule, no crop); pred cleaned as metric.py:98-101; n valid pixels, n = 0 -> NaN everywhere
#   key     uncert, +inf where count < min_count; a NaN orders last (np.sort)
#   terms   fp32: e_rel = |gt - pred| / gt, e_sq = (gt - pred)^2
#   level k (0 .. L - 1) of a key set K: n_k = n - floor(n k / L), t_k = the n_k-th smallest key, S_k = {i valid: K_i <= t_k} -- ties
#           are kept, so no tie-break exists; every key is <= a NaN t_k
#   spars_abs_rel[k] = mean e_rel over S_k, spars_rmse[k] = sqrt(mean e_sq over S_k) with K = key; oracle_abs_rel with K = e_rel,
#   oracle_rmse with K = e_sq; kept[k] = |S_k| / n (K = key); sums in float64
#   ause_X = mean_k(spars_X[k] - oracle_X[k]); aurg_X = mean_k(spars_X[0] - spars_X[k])
# ------------------------------------------------------------------------------------------------------------------
UNCERT_KEYS = ("ause_abs_rel", "aurg_abs_rel", "ause_rmse", "aurg_rmse")
UNCERT_CURVES = ("spars_abs_rel", "spars_rmse", "oracle_abs_rel", "oracle_rmse", "kept")
UNCERT_MAX_LEVELS = 64


def _check_levels(levels) -> int:
    levels = int(levels)
    if not 1 <= levels <= UNCERT_MAX_LEVELS:
        raise ValueError(f"levels = {levels} out of range [1, {UNCERT_MAX_LEVELS}]")
    return levels


def _uncertainty_result(c: dict, curves: bool) -> dict:
    """the four scores from the five curves (NaN curves: n = 0)"""
    out = {}
    with np.errstate(invalid="ignore"):
        for x in ("abs_rel", "rmse"):
            sp, orc = c["spars_" + x], c["oracle_" + x]
            out["ause_" + x] = float(np.mean(sp - orc))
            out["aurg_" + x] = float(np.mean(sp[0] - sp))
    out = {k: out[k] for k in UNCERT_KEYS}
    if curves:
        out.update(c)
    return out


def _empty_curves(levels) -> dict:
    c = {k: np.full(levels, np.nan) for k in UNCERT_CURVES}
    c.update(thresholds=np.full((3, levels), np.nan, np.float32), kept_count=np.zeros(levels, np.int64), n=0)
    return c


def compute_uncertainty_metrics(gt, pred, uncert, count=None, min_count=0, min_depth_eval=0.1, max_depth_eval=10, levels=20, curves=False):
    """AUSE / AURG of one frame on the host (numpy only, fp32 terms, float64 sums): ``ause_abs_rel, aurg_abs_rel, ause_rmse,
    aurg_rmse`` by the definition above, through np.sort.  ``curves=True`` adds the five arrays [L] ``spars_abs_rel, spars_rmse,
    oracle_abs_rel, oracle_rmse, kept`` and, for whoever checks a device route against this one, ``thresholds`` (fp32 [3, L]: the t_k of
    the uncertainty, e_rel and e_sq ordering), ``kept_count`` (int64 [L]) and ``n``.

    This function is NOT in the reference (its tester only writes the uncertainty maps, tester.py:132-181), so no golden file from the
    reference can exist: this numpy statement IS the oracle of the device route, checked in tests/test_uncert_eval_host.py against a
    literal stable-argsort implementation."""
    levels = _check_levels(levels)

    def f32(x):
        x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
        return np.array(x, dtype=np.float32).reshape(x.shape[-2:])  # (a copy: the cleaning below writes into it)
    g, p, u = f32(gt), f32(pred), f32(uncert)
    c = None if count is None else f32(count)
    for name, t in (("pred", p), ("uncert", u), ("count", c)):
        if t is not None and t.shape != g.shape:
            raise ValueError(f"compute_uncertainty_metrics: {name} {t.shape} does not match gt {g.shape}: resize the maps to one shape first")
    mn, mx = np.float32(min_depth_eval), np.float32(max_depth_eval)
    with np.errstate(invalid="ignore"):
        valid = (g > mn) & (g < mx)
        p[p < mn] = mn           # metric.py:98-101, in its order
        p[p > mx] = mx
        p[np.isinf(p)] = mx
        p[np.isnan(p)] = mn
        if c is not None:
            u[c.astype(np.float64) < float(min_count)] = np.inf
    n = int(valid.sum())
    if n == 0:
        return _uncertainty_result(_empty_curves(levels), curves)
    g, p, key = g[valid], p[valid], u[valid]
    d = g - p                     # fp32 throughout
    e_rel, e_sq = np.abs(d) / g, d * d
    rel64, sq64 = e_rel.astype(np.float64), e_sq.astype(np.float64)

    def kept_sets(K):
        srt = np.sort(K)          # NaN last
        with np.errstate(invalid="ignore"):
            for k in range(levels):
                t = srt[n - (n * k) // levels - 1]
                yield t, (np.isnan(t) | (K <= t))
    out = {k: np.empty(levels) for k in UNCERT_CURVES}
    out.update(thresholds=np.empty((3, levels), np.float32), kept_count=np.empty(levels, np.int64), n=n)
    for k, (t, keep) in enumerate(kept_sets(key)):
        m = int(keep.sum())
        out["thresholds"][0, k], out["kept_count"][k], out["kept"][k] = t, m, m / n
        out["spars_abs_rel"][k], out["spars_rmse"][k] = rel64[keep].sum() / m, np.sqrt(sq64[keep].sum() / m)
    for k, (t, keep) in enumerate(kept_sets(e_rel)):
        out["thresholds"][1, k], out["oracle_abs_rel"][k] = t, rel64[keep].sum() / keep.sum()
    for k, (t, keep) in enumerate(kept_sets(e_sq)):
        out["thresholds"][2, k], out["oracle_rmse"][k] = t, np.sqrt(sq64[keep].sum() / keep.sum())
    return _uncertainty_result(out, curves)


def uncertainty_from_values(v, levels, curves=False) -> dict:
    """one frame's row of ops.sparsify (include/prv2.h prv2_sparsify) -> the dict of compute_uncertainty_metrics"""
    L = _check_levels(levels)
    v = np.asarray(v, dtype=np.float64)
    n = int(v[0])
    if n == 0:
        return _uncertainty_result(_empty_curves(L), curves)
    thr, q = v[1:1 + 3 * L].reshape(3, L), v[1 + 3 * L:1 + 10 * L].reshape(7, L)
    c = dict(spars_abs_rel=q[1] / q[0], spars_rmse=np.sqrt(q[2] / q[0]), oracle_abs_rel=q[4] / q[3], oracle_rmse=np.sqrt(q[6] / q[5]),
             kept=q[0] / n, thresholds=thr.astype(np.float32), kept_count=q[0].astype(np.int64), n=n)
    return _uncertainty_result(c, curves)


@torch.no_grad()
def compute_uncertainty_metrics_fused(gt: torch.Tensor, pred: torch.Tensor, uncert: torch.Tensor, count=None, min_count=0, min_depth_eval=0.1,
                                      max_depth_eval=10, levels=20, curves=False):
    """``compute_uncertainty_metrics`` on the GPU (csrc/sparsify.hip, ops.sparsify): fp32 GPU tensors [H, W] / [1, 1, H, W] (a dict) or
    [B, H, W] / [B, 1, H, W] (a list of dicts), all of one shape; ONE D2H of 1 + 10 L float64 values per frame.  The thresholds are
    the exact order statistics of the radix select behind ops.order_stats."""
    from . import ops
    levels = _check_levels(levels)
    maps = dict(gt=gt, pred=pred, uncert=uncert, count=count)
    for name, t in maps.items():
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda):
            raise ValueError(f"compute_uncertainty_metrics_fused: {name} must be a GPU tensor (compute_uncertainty_metrics is the host's)")
        if t is not None and tuple(t.shape[-2:]) != tuple(gt.shape[-2:]):
            raise ValueError(f"compute_uncertainty_metrics_fused: {name} {tuple(t.shape)} does not match gt {tuple(gt.shape)}: "
                             "resize the maps to one shape first")
    g, single = _frames_of(gt)
    rest = [None if t is None else t.reshape(-1, t.shape[-2], t.shape[-1]) for t in (pred, uncert, count)]
    vals = ops.sparsify(g, *rest, min_count=min_count, min_depth=min_depth_eval, max_depth=max_depth_eval, levels=levels).cpu().numpy()  # the one D2H
    rows = [uncertainty_from_values(v, levels, curves) for v in vals]
    return rows[0] if single else rows


def evaluate(per_frame: list) -> dict:
    """mean of every metric over the frames (general_dataset.py evaluate / mmengine-style collect).  The boundary F1 keys
    (BOUNDARY_KEYS, and their coarse_ twins) skip a frame whose score is NaN -- one without a valid pair; NaN when no frame is left."""
    def mean(k):
        v = [float(m[k]) for m in per_frame]
        if k.endswith(BOUNDARY_KEYS):
            v = [x for x in v if not np.isnan(x)] or [float("nan")]
        return float(np.mean(v))
    return {k: mean(k) for k in per_frame[0].keys()}


def colorize(value, vmin=None, vmax=None, cmap="turbo_r", invalid_val=-99, invalid_mask=None,
             background_color=(128, 128, 128, 255), gamma_corrected=False, value_transform=None, vminp=2, vmaxp=95):
    """[H,W] / [1,1,H,W] depth -> RGBA uint8 [H,W,4]."""
    import matplotlib
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    value = value.squeeze()
    if invalid_mask is None:
        invalid_mask = value == invalid_val
    mask = np.logical_not(invalid_mask)
    vmin = np.percentile(value[mask], vminp) if vmin is None else vmin
    vmax = np.percentile(value[mask], vmaxp) if vmax is None else vmax
    value = (value - vmin) / (vmax - vmin) if vmin != vmax else value * 0.0
    value[invalid_mask] = np.nan
    if value_transform:
        value = value_transform(value)
    img = matplotlib.colormaps[cmap](value, bytes=True)
    img[invalid_mask] = background_color
    if gamma_corrected:
        img = (np.power(img / 255, 2.2) * 255).astype(np.uint8)
    return img


# ------------------------------------------------------------------------------------------------------------------
# <name>_edge.png of the tester's output stage (estimator/tester/tester.py:99-106): Canny edges of the LOG depth
# (extract_edges(result, use_canny=True, preprocess='log'), estimator/utils/metric.py:169-207), widened by one pixel
# (kornia.filters.gaussian_blur2d(edges, (3, 3), ...) > 0 == a 3 x 3 binary dilation).
# skimage.feature.canny and kornia are not vendored in the reference nor installed here: the detector below restates
# skimage's published algorithm on scipy.ndimage (what skimage itself is built on) -- PARITY UNPINNED.
# ------------------------------------------------------------------------------------------------------------------
def canny(image: np.ndarray, sigma: float = 1.0, low_threshold: float = 0.1, high_threshold: float = 0.2) -> np.ndarray:
    """skimage.feature.canny(image, sigma) with its defaults (mode='constant', cval=0, thresholds 0.1 / 0.2, no mask):
    Gaussian smoothing corrected for the zero border ("bleed-over"), Sobel gradients, non-maximum suppression with
    bilinear interpolation along the gradient in four 45-degree sectors, hysteresis = 8-connected components of the
    low-threshold maxima that contain a high-threshold pixel."""
    from scipy import ndimage as ndi
    image = np.asarray(image, dtype=np.float32)
    ones = np.ones(image.shape, dtype=np.float32)
    bleed = ndi.gaussian_filter(ones, sigma, mode="constant", cval=0.0) + np.finfo(np.float32).eps
    smoothed = ndi.gaussian_filter(image, sigma, mode="constant", cval=0.0) / bleed
    eroded = np.ones(image.shape, dtype=bool)
    eroded[:1, :] = eroded[-1:, :] = False
    eroded[:, :1] = eroded[:, -1:] = False
    jsobel = ndi.sobel(smoothed, axis=1)
    isobel = ndi.sobel(smoothed, axis=0)
    magnitude = np.sqrt(isobel * isobel + jsobel * jsobel)
    ai, aj = np.abs(isobel), np.abs(jsobel)
    eroded = eroded & (magnitude >= low_threshold)
    local_max = np.zeros(image.shape, dtype=bool)

    def sector(pts, a_slice, b_slice, pa, pb, c_slice, d_slice, pc, pd, w_num, w_den):
        pts = eroded & pts
        m = magnitude[pts]
        w = w_num[pts] / w_den[pts]
        c1, c2 = magnitude[a_slice][pts[pa]], magnitude[b_slice][pts[pb]]
        plus = c2 * w + c1 * (1 - w) <= m
        c1, c2 = magnitude[c_slice][pts[pc]], magnitude[d_slice][pts[pd]]
        minus = c2 * w + c1 * (1 - w) <= m
        local_max[pts] = plus & minus

    s = np.s_
    same = ((isobel >= 0) & (jsobel >= 0)) | ((isobel <= 0) & (jsobel <= 0))
    opp = ((isobel <= 0) & (jsobel >= 0)) | ((isobel >= 0) & (jsobel <= 0))
    # 0 - 45 degrees: neighbours (i+1, j) / (i+1, j+1) and (i-1, j) / (i-1, j-1)
    sector(same & (ai >= aj), s[1:, :], s[1:, 1:], s[:-1, :], s[:-1, :-1], s[:-1, :], s[:-1, :-1], s[1:, :], s[1:, 1:], aj, ai)
    # 45 - 90: (i, j+1) / (i+1, j+1) and (i, j-1) / (i-1, j-1)
    sector(same & (ai <= aj), s[:, 1:], s[1:, 1:], s[:, :-1], s[:-1, :-1], s[:, :-1], s[:-1, :-1], s[:, 1:], s[1:, 1:], ai, aj)
    # 90 - 135: (i, j+1) / (i-1, j+1) and (i, j-1) / (i+1, j-1)
    sector(opp & (ai <= aj), s[:, 1:], s[:-1, 1:], s[:, :-1], s[1:, :-1], s[:, :-1], s[1:, :-1], s[:, 1:], s[:-1, 1:], ai, aj)
    # 135 - 180: (i-1, j) / (i-1, j+1) and (i+1, j) / (i+1, j-1)
    sector(opp & (ai >= aj), s[:-1, :], s[:-1, 1:], s[1:, :], s[1:, :-1], s[1:, :], s[1:, :-1], s[:-1, :], s[:-1, 1:], aj, ai)
    low_mask = local_max & (magnitude >= low_threshold)
    labels, count = ndi.label(low_mask, np.ones((3, 3), bool))
    if count == 0:
        return low_mask
    high_mask = low_mask & (magnitude >= high_threshold)
    good = np.zeros((count + 1,), bool)
    good[np.unique(labels[high_mask])] = True
    good[0] = False
    return good[labels]


def depth_edges(depth) -> np.ndarray:
    """the boolean map behind <name>_edge.png: canny(log depth) dilated 3 x 3 (tester.py:99-105)"""
    from scipy import ndimage as ndi
    d = torch.as_tensor(depth).detach().cpu().float().squeeze()
    d = (d > 0) * d.clamp(min=torch.finfo(torch.float32).eps).log()  # to_log, metric.py:157-161
    return ndi.binary_dilation(canny(d.numpy(), sigma=1.0), structure=np.ones((3, 3), bool))


# ------------------------------------------------------------------------------------------------------------------
# Edge-aware evaluation (host restatements: the spec of csrc/edges.hip and its CPU oracle).
#   extract_edges             estimator/utils/metric.py:169-207
#   compute_boundary_metrics  estimator/utils/metric.py:210-272 (called by cityscapes_dataset.py:340-403)
#   edge_split_masks          scannet_dataset.py:221-224 (the edge_* / noedge_* regions)
# Pinned by tests/golden/edge_metrics.npz (tools/make_edge_golden.py runs the reference's own functions).
# ------------------------------------------------------------------------------------------------------------------
LOG_1_5_F32 = float(np.float32(np.log(1.5)))  # torch.log(torch.tensor(1.5)) (float32)


def gaussian_weights(sigma: float = 1.0) -> np.ndarray:
    """scipy.ndimage's Gaussian taps for gaussian_filter(sigma) (truncate 4): float64, centre first -> [radius + 1]
    (the same expression as scipy's _gaussian_kernel1d, so the same float64 values)"""
    sd = float(sigma)
    radius = int(4.0 * sd + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sd * sd) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[radius:], dtype=np.float64)


def preprocess_depth(depth, preprocess=None) -> np.ndarray:
    """extract_edges' preprocessing (metric.py:184-198) on a float32 map -> float32 numpy"""
    if preprocess not in {"log", "inv", "none", None}:
        raise ValueError(f"Invalid depth preprocessing. ({preprocess})")
    d = torch.as_tensor(np.asarray(depth.detach().cpu() if isinstance(depth, torch.Tensor) else depth)).float().squeeze()
    eps = torch.finfo(torch.float32).eps
    if preprocess == "log":  # to_log (metric.py:155-159)
        d = (d > 0) * d.clamp(min=eps).log()
    elif preprocess == "inv":  # to_inv (metric.py:161-165), then -= min, /= max
        d = (d > 0) / d.clamp(min=eps)
        d -= d.min()
        d /= d.max()
    else:  # 'none' / None: log base 1.5 of the clamped depth (log(0) = -inf where depth <= 0: the reference's quirk)
        d = torch.log((d > 0) * d.clamp(min=eps)) / torch.log(torch.tensor(1.5))
    return d.numpy()


def extract_edges(depth, preprocess=None, sigma=1, mask=None) -> np.ndarray:
    """metric.py:169-207 (use_canny=True): preprocess, then ``canny(., sigma)`` -> bool [H, W]"""
    if mask is not None:
        raise NotImplementedError("extract_edges(mask=...): no caller of the reference passes a mask")
    return canny(preprocess_depth(depth, preprocess), sigma=sigma)


def binary_dilate(edges, k: int) -> np.ndarray:
    """k x k binary dilation, zero padding.  kornia.filters.gaussian_blur2d(e, (k, k), sigma, border_type='reflect') > 0 is
    exactly this: every Gaussian weight is positive, and a reflected tap (pad (k-1)/2, 'reflect' excludes the edge pixel)
    lands inside the same k x k window, so the blur is > 0 iff a set pixel lies in the in-bounds window."""
    from scipy import ndimage as ndi
    return ndi.binary_dilation(np.asarray(edges, bool), structure=np.ones((k, k), bool))


def _np_bool(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x).squeeze().astype(bool)


def binary_scores(tp, fp, fn, tn) -> dict:
    """torchmetrics' BinaryPrecision / Recall / F1Score / HammingDistance / Accuracy from the confusion counts (the reference's
    metric_dict, cityscapes_dataset.py:78-82; torchmetrics is absent): a zero denominator gives 0"""
    tp, fp, fn, tn = (float(v) for v in (tp, fp, fn, tn))
    n = tp + fp + fn + tn

    def div(a, b):
        return a / b if b else 0.0
    return dict(precision=div(tp, tp + fp), recall=div(tp, tp + fn), f1_score=div(2 * tp, 2 * tp + fp + fn), hamming=div(fp + fn, n),
                acc=div(tp + tn, n))


def compute_boundary_metrics(gt_edges, pred_edges, valid_mask, th_edges_acc=10, th_edges_comp=10) -> dict:
    """metric.py:210-272 with its quirks: both distance transforms on the UNMASKED edge maps (masks applied after); EdgeAcc =
    mean D_target over pred & valid & (D_target < th_acc), th_acc when empty; EdgeComp = mean D_pred over ALL valid gt edges,
    guarded by the pred BDE set being non-empty (:245); the F1 family on the 5 x 5-dilated unmasked maps at the valid pixels."""
    from scipy import ndimage as ndi
    gt, pred, valid = _np_bool(gt_edges), _np_bool(pred_edges), _np_bool(valid_mask)
    d_target = ndi.distance_transform_edt(np.logical_not(gt))
    d_pred = ndi.distance_transform_edt(np.logical_not(pred))
    gt_m, pred_m = gt & valid, pred & valid
    pred_bde = pred_m & (d_target < th_edges_acc)
    out = dict(EdgeAcc=float(d_target[pred_bde].mean()) if pred_bde.sum() else float(th_edges_acc),
               EdgeComp=float(d_pred[gt_m].mean()) if pred_bde.sum() else float(th_edges_comp))
    ge, pe = binary_dilate(gt, 5)[valid], binary_dilate(pred, 5)[valid]
    tp, fp, fn = int((pe & ge).sum()), int((pe & ~ge).sum()), int((~pe & ge).sum())
    out.update(binary_scores(tp, fp, fn, int(ge.size) - tp - fp - fn))
    return out


def edge_split_masks(gt, k: int = 7) -> np.ndarray:
    """scannet_dataset.py:221-224: Canny of the log ground truth, widened by gaussian_blur2d((7, 7), sigma 5, reflect) > 0, which
    is the 7 x 7 binary dilation (binary_dilate) -> bool [H, W]; the noedge region is its complement"""
    return binary_dilate(extract_edges(gt, "log"), k)


# KittiDataset's / ScanNetDataset's ground truth on the host (the spec of ops.depth16_gt).
def pil_nearest_index(n_out: int, n_in: int) -> np.ndarray:
    """the source index of every output index of PIL's ``Image.resize(size, Image.NEAREST)`` along one axis -> int64 [n_out]:
    floor((i + 0.5) * (n_in / n_out)), the scale ONE float64 division and every index ONE float64 product (checked against Pillow in
    tests/test_kitti_scannet_host.py; adding the step up instead of multiplying picks other pixels).  Equal sizes: the identity."""
    if n_out < 1 or n_in < 1:
        raise ValueError(f"pil_nearest_index: {n_in} -> {n_out}")
    scale = np.float64(n_in) / np.float64(n_out)
    return np.minimum(((np.arange(n_out, dtype=np.float64) + 0.5) * scale).astype(np.int64), n_in - 1)


def depth16_decode_spec(samples, divisor, window=None, out_hw=None, th=1.0):
    """the uint16 samples [sh, sw] of a depth PNG -> (depth float32, boundary uint8) as the reference makes them:
    ``window=(top, left, h, w)``: ``Image.crop`` (kitti_dataset.py:123-131; None with ``out_hw`` None: the whole map); ``out_hw=(H, W)``:
    ``Image.resize((W, H), Image.NEAREST)`` (scannet_dataset.py:112-118); depth = samples.astype(float32) / divisor (kitti_dataset.py:142
    with 256.0, scannet_dataset.py:132 with 1000.0); boundary = get_boundaries(depth, th, dilation=0) of THAT map (:203 / :188)."""
    s = np.asarray(samples)
    if s.dtype != np.uint16 or s.ndim != 2:
        raise ValueError(f"depth16_decode_spec: samples are uint16 [H, W], not {s.dtype} {s.shape}")
    if window is not None and out_hw is not None:
        raise ValueError("depth16_decode_spec: give window or out_hw, not both")
    if window is not None:
        top, left, h, w = (int(v) for v in window)
        if top < 0 or left < 0 or h < 1 or w < 1 or top + h > s.shape[0] or left + w > s.shape[1]:
            raise ValueError(f"depth16_decode_spec: the window of {h} x {w} at ({top}, {left}) lies outside the {s.shape[0]} x {s.shape[1]} map")
        s = s[top:top + h, left:left + w]
    elif out_hw is not None:
        s = s[pil_nearest_index(int(out_hw[0]), s.shape[0])[:, None], pil_nearest_index(int(out_hw[1]), s.shape[1])[None, :]]
    depth = s.astype(np.float32) / np.float32(divisor)
    return depth, get_boundaries(depth, th=np.float32(th), dilation=0).astype(np.uint8)


# CityScapesDataset.get_metrics' pixel sets (host restatements: the spec of ops.seg_canny / ops.cityscapes_masks).
#   seg_canny         cityscapes_dataset.py:333-334 (kornia.filters.canny on the colour segmentation map) -- kornia is not installed:
#                     PARITY UNPINNED, as for ``canny`` above; this restatement is the specification
#   cityscapes_masks  cityscapes_dataset.py:360-365
SEG_CANNY_TAN_PI_8 = np.float32(np.tan(np.pi / 8))  # the half width of a 45-degree sector


def seg_canny_weights() -> np.ndarray:
    """kornia's 5-tap Gaussian of sigma 1 (get_gaussian_kernel1d: exp(-x^2 / (2 sigma^2)) normalised by its sum) in float32 -> [5]"""
    x = torch.arange(5, dtype=torch.float32) - 2
    g = torch.exp(-x.pow(2.0) / (2 * 1.0 ** 2))
    return np.ascontiguousarray((g / g.sum()).numpy(), dtype=np.float32)


def seg_canny_axis(gx: np.ndarray, gy: np.ndarray) -> np.ndarray:
    """the axis kornia's non-maximum suppression compares along, without atan2: 0 horizontal, 1 vertical, 2 the (+1, +1) diagonal,
    3 the (+1, -1) diagonal.  kornia rounds atan2(gy, gx) to a multiple of 45 degrees and looks at the neighbour in that direction
    and the opposite one, so this is round(atan2 * 4 / pi) mod 4.  float32 in, one float32 product per comparison."""
    a, b = np.abs(gx), np.abs(gy)
    T = SEG_CANNY_TAN_PI_8
    return np.where(b <= T * a, 0, np.where(a <= T * b, 1, np.where((gx > 0) == (gy > 0), 2, 3))).astype(np.uint8)


def seg_canny_hysteresis(weak: np.ndarray, strong: np.ndarray) -> np.ndarray:
    """the fixed point of kornia's hysteresis loop: the strong pixels, and the weak pixels 8-connected to one through weak pixels
    (``strong`` is a subset of ``weak``)"""
    from scipy import ndimage as ndi
    labels, count = ndi.label(weak, np.ones((3, 3), bool))
    good = np.zeros((count + 1,), bool)
    good[np.unique(labels[strong])] = True
    good[0] = False
    return good[labels]


def seg_canny_magnitude(seg):
    """steps 1-5 of ``seg_canny`` -> (mag float32 [H, W], axis uint8 [H, W])"""
    s = np.asarray(seg.detach().cpu() if isinstance(seg, torch.Tensor) else seg, dtype=np.float32)
    s = s.reshape(3, *s.shape[-2:])
    h, w = s.shape[1:]
    if h < 3 or w < 3:
        raise ValueError(f"seg_canny: {h} x {w}: the reflect pad of 2 needs at least 3 x 3 pixels")
    f = np.float32
    grey = (f(0.299) * s[0] + f(0.587) * s[1]) + f(0.114) * s[2]
    g = seg_canny_weights()
    p = np.pad(grey, ((0, 0), (2, 2)), mode="reflect")
    t = g[0] * p[:, 0:w]
    for j in range(1, 5):
        t = t + g[j] * p[:, j:j + w]
    p = np.pad(t, ((2, 2), (0, 0)), mode="reflect")
    sm = g[0] * p[0:h]
    for j in range(1, 5):
        sm = sm + g[j] * p[j:j + h]
    p = np.pad(sm, 1, mode="edge")
    u, c, d = p[0:h], p[1:h + 1], p[2:h + 2]  # the rows above, at and below; columns x - 1, x, x + 1 at 0:w, 1:w + 1, 2:w + 2
    gx = ((u[:, 2:] - u[:, :w]) + f(2) * (c[:, 2:] - c[:, :w])) + (d[:, 2:] - d[:, :w])
    gy = ((d[:, :w] - u[:, :w]) + f(2) * (d[:, 1:w + 1] - u[:, 1:w + 1])) + (d[:, 2:] - u[:, 2:])
    mag = np.sqrt((gx * gx + gy * gy) + f(1e-6))
    assert mag.dtype == np.float32
    return mag, seg_canny_axis(gx, gy)


def seg_canny(seg, low_threshold=0.1, high_threshold=0.2) -> np.ndarray:
    """cityscapes_dataset.py:333-334: ``kornia.filters.canny(seg)[1] > 0`` with kornia's defaults on the colour segmentation map
    [3, H, W] (or [1, 3, H, W]) -> bool [H, W].  float32 throughout, as shifted sums in a fixed order and never as a convolution call --
    on an axis-aligned class boundary the two pixels beside the step have mathematically equal magnitudes, so the strict > of step 6
    is decided by the last bit and the operation order IS the specification (include/prv2.h prv2_seg_canny repeats it):
      1 grey = (0.299 R + 0.587 G) + 0.114 B            2 5-tap Gaussian of sigma 1 along x, then y; reflect border; taps -2 .. +2
      3 unnormalised Sobel, replicate border              4 mag = sqrt((gx gx + gy gy) + 1e-6)
      5 the axis of the gradient (seg_canny_axis)         6 maximum iff min(mag - n1, mag - n2) > 0, 0 outside the frame
      7 strong = maximum and mag > high, weak = maximum and mag > low; the result is seg_canny_hysteresis(weak, strong)"""
    mag, axis = seg_canny_magnitude(seg)
    h, w = mag.shape
    p = np.pad(mag, 1)  # zero outside the frame

    def nb(dy, dx):
        return p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    steps = ((0, 1), (1, 0), (1, 1), (-1, 1))  # (dy, dx) of the axes 0 .. 3
    is_max = np.zeros((h, w), bool)
    for k, (dy, dx) in enumerate(steps):
        is_max |= (axis == k) & (np.minimum(mag - nb(dy, dx), mag - nb(-dy, -dx)) > 0)
    weak = is_max & (mag > np.float32(low_threshold))
    return seg_canny_hysteresis(weak, weak & (mag > np.float32(high_threshold)))


def cityscapes_masks(seg_edges, gt_edges, hr_region):
    """cityscapes_dataset.py:360-365 without the valid-depth mask (the scoring applies it) -> (edge_mask, flatten), bool [H, W]:
    edge_mask = seg edges and the 7 x 7-widened ground-truth depth edges (``binary_dilate``: the blur > 0), flatten = not edge_mask
    and not the image-edge region"""
    def m(x):  # ([H, W] stays [H, W], also for H = W = 1)
        x = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
        return x.reshape(x.shape[-2:]).astype(bool)
    edge = m(seg_edges) & binary_dilate(m(gt_edges), 7)
    return edge, ~edge & ~m(hr_region)


# device route (csrc/edges.hip through ops.py): the same functions on GPU tensors, B frames per call
def _frames_of(x: torch.Tensor):
    """[H, W] / [1, 1, H, W] -> ([1, H, W], True); [B, H, W] / [B, 1, H, W] -> ([B, H, W], False)"""
    single = x.dim() == 2 or (x.dim() == 4 and x.shape[0] == 1)
    return x.reshape(-1, x.shape[-2], x.shape[-1]), single


@torch.no_grad()
def extract_edges_device(depth: torch.Tensor, preprocess="log", sigma=1) -> torch.Tensor:
    """``extract_edges`` on the device: bool [H, W] for one map ([H, W] or [1, 1, H, W]), [B, H, W] for B maps"""
    from . import ops
    x, single = _frames_of(depth)
    e = ops.canny(ops.depth_preprocess(x.float(), preprocess), sigma=sigma)
    return e[0] if single else e


def _boundary_dict(s, th_edges_acc, th_edges_comp) -> dict:
    tp, fp, fn, tn, n_bde, n_gt, sum_acc, sum_comp = s
    out = dict(EdgeAcc=sum_acc / n_bde if n_bde else float(th_edges_acc),
               EdgeComp=(sum_comp / n_gt if n_gt else float("nan")) if n_bde else float(th_edges_comp))
    out.update(binary_scores(tp, fp, fn, tn))
    return out


@torch.no_grad()
def compute_boundary_metrics_device(gt_edges: torch.Tensor, pred_edges: torch.Tensor, valid_mask: torch.Tensor, th_edges_acc=10,
                                    th_edges_comp=10):
    """``compute_boundary_metrics`` on the device (two exact distance transforms, two 5 x 5 dilations, one statistics pass; one D2H
    of the scalars): a dict for one map, a list of dicts for [B, H, W]"""
    from . import ops
    g, single = _frames_of(gt_edges.bool())
    p, v = pred_edges.bool().reshape(g.shape), valid_mask.bool().reshape(g.shape)
    stats = ops.boundary_stats(g, p, v, ops.edt_sq(g), ops.edt_sq(p), ops.binary_dilate(g, 5), ops.binary_dilate(p, 5), th_edges_acc)
    rows = [_boundary_dict(r, th_edges_acc, th_edges_comp) for r in stats.cpu().tolist()]
    return rows[0] if single else rows


@torch.no_grad()
def edge_split_masks_device(gt: torch.Tensor, k: int = 7) -> torch.Tensor:
    """``edge_split_masks`` on the device"""
    from . import ops
    e = extract_edges_device(gt, "log")
    d = ops.binary_dilate(e, k)
    return d[0] if e.dim() == 2 else d
