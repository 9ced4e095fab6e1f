"""GPU: the scale-invariant boundary F1 -- csrc/boundary_eval.hip (both dispatch routes) against the counts of the numpy specification
(metrics.compute_boundary_f1, pinned by tests/test_boundary_f1_host.py), its bit-exactness properties (call to call, alone or in a
batch, resize inside or before the kernel, crop or zeroed ground truth, torch op or C ABI), get_metrics(boundary_f1=True) of three
datasets over tiny synthetic trees and the coarse prediction's scores of Tester.run.

Every comparison is exact equality of the integer rows: the counts are integers, both sides decide every flag by the same fp32
compare-after-multiply, so there is no tolerance."""
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_boundary_f1_host import BOUNDARY_KEYS, MN, MX, PLAIN, frame, spec  # noqa: E402
from test_eth_dataset_host import _dataset as eth_dataset, write_eth_tree  # noqa: E402
from test_general_gt_host import _dataset as general_dataset, write_general_tree  # noqa: E402
from test_u4k_eval_gpu import RAW, SPLIT, _write_cfg, route  # noqa: E402,F401
from test_u4k_eval_host import _dataset as u4k_dataset, write_u4k_tree  # noqa: E402

DEV = "cuda"
GARG = (15, 36, 1, 51)  # metrics._eval_crop(37, 53, garg_crop=True)
torch.set_grad_enabled(False)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def counts(ops, gt, pred, crop=None, thresholds=None):
    """one frame's row of the op as a list"""
    out = ops.boundary_f1(dev(gt)[None], dev(pred)[None], MN, MX, crop, thresholds)
    assert out.dtype == torch.float64 and out.is_cuda and out.shape[0] == 1
    return out[0].cpu().numpy().tolist()


_FRAMES = {}


def case(shape):
    """the frame of a shape and the specification's row for it, computed once"""
    if shape not in _FRAMES:
        gt, pred = frame(shape, 200 + shape[0] * 3 + shape[1])
        if shape == (64, 1028):  # a ground-truth and a prediction boundary across the 1024-column block border, in every row
            gt[:, 1020:1024], gt[:, 1024:] = 1.0, 3.0
            pred[:, 1023], pred[:, 1024] = 2.0, 1.0
        _FRAMES[shape] = (gt, pred, spec(gt, pred)[1].tolist())
    return _FRAMES[shape]


# ------------------------------------------------------------------------------------------------------------------ against the specification
# no pair; no vertical pair; no horizontal pair; tiny; scalar tail; holes; across the column-block border and quads; many row blocks
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 5), (5, 9), (37, 53), (64, 1028), (270, 480)])
def test_op_against_the_specifications_counts(route, shape):  # noqa: F811
    gt, pred, want = case(shape)
    got = counts(route, gt, pred)
    assert len(got) == 122 and got == want, (shape, got[:14], want[:14])
    assert got == counts(route, gt, pred)  # the same bits on every call
    if min(shape) > 1:
        assert want[0] > 0 and want[1] > 0 and max(want[2:]) > 0
    if shape == (64, 1028):
        c = np.asarray(want[2:]).reshape(10, 4, 3)
        assert c[0, 2, 2] >= 64 and c[0, 0, 1] >= 64  # the pairs across the block border are counted (R in gt, L in the prediction)


def test_crop_with_holes_against_the_specification(route):  # noqa: F811
    gt, pred, whole = case((37, 53))
    want = spec(gt, pred, garg_crop=True)[1].tolist()
    assert counts(route, gt, pred, GARG) == want and want != whole and want[0] > 0


def test_other_threshold_counts_and_orders(route):  # noqa: F811
    gt, pred, _ = case((37, 53))
    for th in ((1.3,), (1.25, 1.05, 1.5), tuple(np.linspace(1.02, 2.0, 16))):
        got = counts(route, gt, pred, thresholds=th)
        assert len(got) == 2 + 12 * len(th) and got == spec(gt, pred, thresholds=th)[1].tolist(), th


def test_unaligned_base_pointer_takes_the_scalar_loads(route):  # noqa: F811
    gt, pred, want = case((64, 1028))
    bufs = [torch.zeros(1 + gt.size, dtype=torch.float32, device=DEV) for _ in range(2)]
    views = []
    for buf, a in zip(bufs, (gt, pred)):
        v = buf[1:].view(1, *gt.shape)  # a view offset by one float: rows are not 16-byte aligned
        v.copy_(dev(a)[None])
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        views.append(v)
    assert route.boundary_f1(*views, MN, MX)[0].cpu().numpy().tolist() == want


# ------------------------------------------------------------------------------------------------------------------ bit-exactness
def three_frames(shape):
    """the shape's frame under three different masks"""
    gt, pred, _ = case(shape)
    h, w = shape
    g = np.stack([gt] * 3)
    g[1, : h // 3] = 0.0
    g[1, :, w // 2:w // 2 + 3] = 20.0
    g[2, ::3, 1::2] = 0.0
    p = np.stack([pred, pred[::-1], pred[:, ::-1]])
    return g, p


@pytest.mark.parametrize("shape", [(37, 53), (270, 480)])
def test_frames_in_a_batch_equal_the_frames_alone(route, shape):  # noqa: F811
    g, p = three_frames(shape)
    out = route.boundary_f1(dev(g), dev(p), MN, MX)
    assert tuple(out.shape) == (3, 122) and len({float(v) for v in out[:, 0]}) == 3
    for f in range(3):
        assert same_bits(route.boundary_f1(dev(g[f:f + 1]), dev(p[f:f + 1]), MN, MX), out[f:f + 1]), (shape, f)
        assert out[f].cpu().numpy().tolist() == spec(g[f], p[f])[1].tolist()
    assert same_bits(route.boundary_f1(dev(g), dev(p), MN, MX), out)


@pytest.mark.parametrize("pshape,shape", [((19, 27), (37, 53)), ((1, 1), (37, 53)), ((80, 96), (37, 53)), ((135, 240), (270, 480))])
def test_resize_inside_the_kernel_equals_interpolate_then_score(route, pshape, shape):  # noqa: F811
    gt, _, whole = case(shape)
    g = dev(gt)[None]
    rs = np.random.RandomState(pshape[0] * 1000 + pshape[1])
    small = dev((0.5 + 8.0 * rs.rand(1, *pshape)).astype(np.float32))
    up = F.interpolate(small[:, None], shape, mode="bilinear", align_corners=False)[:, 0].contiguous()
    crop = GARG if shape == (37, 53) else None
    low = route.boundary_f1(g, small, MN, MX, crop)
    assert same_bits(low, route.boundary_f1(g, up, MN, MX, crop)), (pshape, shape)
    row = low[0].cpu().numpy()
    assert row.tolist() == spec(gt, up[0].cpu().numpy(), garg_crop=crop is not None)[1].tolist()
    assert row[0] > 0 and (pshape == (1, 1)) == (row[2:].reshape(10, 4, 3)[..., 1].max() == 0)  # a 1 x 1 source is a constant map


def test_crop_limits_the_mask_and_the_pairs(route):  # noqa: F811
    from patchrefinerv2_amd import metrics as M
    gt, pred, whole = case((37, 53))
    y0, y1, x0, x1 = GARG
    cropped = counts(route, gt, pred, GARG)
    outside = gt.copy()
    keep = np.zeros(outside.shape, bool)
    keep[y0:y1, x0:x1] = True
    outside[~keep] = 0.0  # the same pixel set without a crop: nothing outside is in the mask, no pair reaches across the border
    assert counts(route, outside, pred) == cropped and cropped != whole
    for crop in ((0, 37, 0, 0), (5, 5, 0, 53)):  # an empty crop: nothing is valid
        row = counts(route, gt, pred, crop)
        assert row == [0.0] * 122
        assert all(np.isnan(v) for v in M.boundary_from_values(row, M.boundary_thresholds()).values())
    fused = M.compute_boundary_f1_fused(dev(gt), dev(pred), **dict(PLAIN, garg_crop=True))
    assert tuple(fused) == BOUNDARY_KEYS and fused == M.compute_boundary_f1(gt, pred, **dict(PLAIN, garg_crop=True))
    rows = M.compute_boundary_f1_fused(dev(np.stack([gt, outside])), dev(np.stack([pred, pred])), curves=True, **PLAIN)
    assert isinstance(rows, list) and rows[0] == spec(gt, pred)[0] and rows[1] == spec(outside, pred)[0]


def test_non_finite_and_negative_prediction_inside_the_mask_is_cleaned(route):  # noqa: F811
    gt, pred, _ = case((37, 53))
    valid = (gt > MN) & (gt < MX)
    p = pred.copy()
    ys, xs = np.nonzero(valid)
    for k, bad in enumerate((np.nan, np.inf, -np.inf, -3.0, 0.0, 1e30)):
        p[ys[5 + 11 * k], xs[5 + 11 * k]] = bad
    want = spec(gt, p)[1].tolist()
    assert counts(route, gt, p) == want
    cleaned = np.clip(np.nan_to_num(p, nan=MN, posinf=np.inf, neginf=-np.inf), np.float32(MN), np.float32(MX)).astype(np.float32)
    assert counts(route, gt, cleaned) == want
    p[~valid] = np.nan  # outside the mask the prediction is never read
    assert counts(route, gt, p) == want


def test_torch_op_and_c_abi_agree_bitwise(monkeypatch):
    from patchrefinerv2_amd import ops
    g, p = three_frames((270, 480))
    g, p = dev(g), dev(p)
    small = p[:, ::2, ::2].contiguous()
    got = {}
    for r in ("ctypes", "torch"):
        monkeypatch.setattr(ops, "DISPATCH", r)
        got[r] = (ops.boundary_f1(g, p, MN, MX), ops.boundary_f1(g, small, MN, MX, (30, 260, 10, 470), (1.5, 1.1, 1.2)))
    assert same_bits(got["ctypes"][0], got["torch"][0]) and same_bits(got["ctypes"][1], got["torch"][1])
    assert tuple(got["torch"][1].shape) == (3, 38) and float(got["torch"][0][:, 2:].max()) > 0


# ------------------------------------------------------------------------------------------------------------------ the datasets
def f64_bits(v):
    return struct.pack("<d", float(v))


def check_dataset(plain, on, **extra):
    """get_metrics with the flag: today's keys bit-equal to the run without it, then the three keys of the specification (on the
    prediction as the device resizes it)"""
    from patchrefinerv2_amd import metrics as M
    try:
        item = plain[0]
        gt = item["depth_gt"]
        assert gt.is_cuda and on[0]["depth_gt"].equal(gt)
        h, w = gt.shape[-2:]
        clean = torch.where((gt > plain.min_depth) & (gt < plain.max_depth), gt, torch.full_like(gt, 3.0))
        yy, xx = torch.meshgrid(torch.arange(h, device=DEV), torch.arange(w, device=DEV), indexing="ij")
        full = clean * (1.0 + 0.2 * torch.sin(xx * 1.7) * torch.cos(yy * 2.3))
        pred = F.interpolate(full, (h // 2 + 1, w // 2 + 3), mode="bilinear", align_corners=False)
        kw = dict(disp_gt_edges=item["boundary"], **{k: item[k] for k in extra})
        a, b = plain.get_metrics(gt, pred, **kw), on.get_metrics(gt, pred, **kw)
        assert tuple(b) == tuple(a) + BOUNDARY_KEYS and len(a) >= 10
        for k in a:
            assert f64_bits(a[k]) == f64_bits(b[k]), k
        up = F.interpolate(pred, (h, w), mode="bilinear", align_corners=False)
        want = M.compute_boundary_f1(gt.cpu(), up.cpu(), garg_crop=False, eigen_crop=False, dataset="", min_depth_eval=plain.min_depth,
                                     max_depth_eval=plain.max_depth)
        assert np.isfinite(list(want.values())).all() and {k: b[k] for k in BOUNDARY_KEYS} == want, (b, want)
        return a, b
    finally:
        for ds in (plain, on):
            if hasattr(ds, "close"):
                ds.close()


def test_image_dataset_get_metrics(tmp_path):
    img_dir, gt_dir, _ = write_general_tree(str(tmp_path), "eth3d", (37, 53), n=1)
    kw = dict(gt_format="eth3d", gt_shape=(37, 53), image_resolution=(37, 53), min_depth=MN, max_depth=MX)
    check_dataset(general_dataset(img_dir, gt_dir, **kw), general_dataset(img_dir, gt_dir, boundary_f1=True, **kw))


def test_u4k_dataset_get_metrics(tmp_path):
    root = str(tmp_path / "u4k")
    split = write_u4k_tree(root, [("00001", "00002", 1000.0, 0.5)], (38, 52))
    check_dataset(u4k_dataset(root, split, (38, 52)), u4k_dataset(root, split, (38, 52), boundary_f1=True))


def test_eth_dataset_get_metrics(tmp_path):
    split, _ = write_eth_tree(str(tmp_path), 1, (30, 44), (37, 53))
    a, _ = check_dataset(eth_dataset(split, gt_shape=(37, 53)), eth_dataset(split, gt_shape=(37, 53), boundary_f1=True), image_hr="image_hr")
    assert len(a) == 30


# ------------------------------------------------------------------------------------------------------------------ the tester
def test_tester_run_scores_the_coarse_prediction_beside_the_result(tmp_path, monkeypatch):
    from patchrefinerv2_amd import metrics as M, models, weights as W  # noqa: F401
    from patchrefinerv2_amd.registry import DATASETS, Config, build_model
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    root = str(tmp_path / "data")
    write_u4k_tree(root, [("00001", "00004", 480.0, 0.35)], RAW, seed=5)
    cfg = Config.fromfile(_write_cfg(tmp_path, root))
    mcfg = cfg.model.to_dict()
    mcfg["config"].update(prec="bf16x3", max_batch=41, n_streams=3)
    model = build_model(mcfg)
    model.load_state_dict(W.synth_state_dict(model.spec(), seed=0), strict=True)
    ds_cfg = dict(cfg.val_dataloader.dataset.to_dict(), image_raw_shape=list(RAW))
    calls = []
    fused = M.compute_boundary_f1_fused

    def recording(gt, pred, **kw):
        calls.append((gt.cpu(), pred.cpu(), kw))
        return fused(gt, pred, **kw)
    monkeypatch.setattr(M, "compute_boundary_f1_fused", recording)
    runs = {}
    for flag in (False, True):
        ds = DATASETS.build(dict(ds_cfg, boundary_f1=True) if flag else ds_cfg)
        runs[flag] = Tester(None, RunnerInfo(), ds, model).run(cai_mode="m1", image_raw_shape=RAW, patch_split_num=SPLIT, seed=621)
        ds.close()
        assert len(calls) == (2 if flag else 0)  # the result's call and one more for the coarse map
    off, on = runs[False][0]["metrics"], runs[True][0]["metrics"]
    coarse_keys = tuple("coarse_" + k for k in BOUNDARY_KEYS)
    assert not any("si_boundary" in k for k in off)
    assert tuple(on) == tuple(off) + BOUNDARY_KEYS + coarse_keys and all(f64_bits(on[k]) == f64_bits(off[k]) for k in off)
    (gt, result, _), (gt_c, coarse, kw_c) = calls
    assert gt_c.equal(gt) and kw_c["fuse_resize"] is True and coarse.shape[-2:] != gt.shape[-2:] and coarse.shape[-2:] != result.shape[-2:]
    args = dict(garg_crop=False, eigen_crop=False, dataset="", min_depth_eval=ds.min_depth, max_depth_eval=ds.max_depth)
    for prefix, pred in (("", result), ("coarse_", coarse)):
        up = F.interpolate(pred.to(DEV).reshape(1, 1, *pred.shape[-2:]), gt.shape[-2:], mode="bilinear", align_corners=False).cpu()
        want = M.compute_boundary_f1(gt, up, **args)
        assert {k: on[prefix + k] for k in BOUNDARY_KEYS} == want and np.isfinite(list(want.values())).all(), prefix
