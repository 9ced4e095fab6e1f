"""GPU: the scale-and-shift-invariant evaluation -- csrc/ssi_eval.hip (both dispatch routes) against the reference's recorded float64
outputs (tests/golden/ssi_eval.npz), its bit-exactness properties (call to call, alone or in a batch, resize inside or before the
kernels, crop or zeroed ground truth, torch op or C ABI), and get_metrics(ssi_metrics=True) of the three datasets over tiny synthetic
trees.

The bound: float64 accumulation of at most 1.3e5 terms is off by at most 1.3e5 x 1.1e-16 = 1.4e-11 relative in the worst case; the
determinant of the normal equations cancels by a factor of about ten at most on these fixtures (the prediction's variance is a tenth
of its squared mean or more, asserted by tools/make_ssi_golden.py), hence rtol 1e-9 on every key."""
import struct

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_eth_dataset_host import _dataset as eth_dataset, write_eth_tree  # noqa: E402
from test_general_gt_host import _dataset as general_dataset, write_general_tree  # noqa: E402
from test_ssi_eval_host import CASES, MN, MX, SCORED, SSI_KEYS, crop_args  # noqa: E402
from test_u4k_eval_gpu import route  # noqa: E402,F401
from test_u4k_eval_host import _dataset as u4k_dataset, write_u4k_tree  # noqa: E402

DEV = "cuda"
RTOL = 1e-9
torch.set_grad_enabled(False)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def score(ops, name, **kw):
    c = CASES[name]
    return ops.ssi_metrics(dev(c["gt"])[None], dev(c["pred"])[None], MN, MX, kw.pop("crop", c["crop"]), **kw)


def close(got, want, what):
    """every key within RTOL; prints the largest relative deviation (collected by tools/bench_ssi_eval.py for profiles/ssi_eval.json)"""
    worst = 0.0
    for k in SSI_KEYS:
        g, w = float(got[k]), float(want[k])
        d = abs(g - w) / abs(w) if w else abs(g)
        worst = max(worst, d)
        print(f"{what} {k}: got {g!r} want {w!r} rel {d:.3e}")
        assert d <= RTOL, (what, k, g, w, d)
    print(f"{what}: largest relative deviation {worst:.3e}")
    return worst


# ------------------------------------------------------------------------------------------------------------------ against the fixture
@pytest.mark.parametrize("name", SCORED)  # 2 x 7 (no vertical pair), 5 x 7, 37 x 53 (+ crop), 270 x 480 (many row blocks), det == 0
def test_op_against_the_reference(route, name):  # noqa: F811
    from patchrefinerv2_amd import metrics as M
    c = CASES[name]
    out = score(route, name)
    assert out.dtype == torch.float64 and tuple(out.shape) == (1, 41) and out.is_cuda
    assert same_bits(score(route, name), out)  # the same bits on every call
    row = out[0].cpu().numpy()
    assert row[6] == c["n"] and row[39] == 0 and row[40] == 0 and row[9] == c["n"] and row[29] == c["n"]
    if c["gt"].shape[0] <= 2:
        assert (row[[2, 3, 23, 25, 27]] == 0).all() and (row[12:17] == 0).all()  # no vertical pair exists
    close(M.ssi_from_values(row), c["want"], f"{route.DISPATCH} {name}")


def test_zero_determinant_and_single_pixel_on_the_device(route):  # noqa: F811
    from patchrefinerv2_amd import metrics as M
    row = score(route, "constpred8x16")[0].cpu().numpy()
    a00, a01, a11 = row[7:10]
    assert a00 * a11 - a01 * a01 == 0.0 and (row[0:2] == 0).all() and row[6] == 128  # det == 0 exactly: no fit
    row = score(route, "single5x7")[0].cpu().numpy()
    assert row[6] == 1 and (row[0:6] == 0).all()  # one sample: det == 0
    m = M.ssi_from_values(row)
    assert tuple(m) == SSI_KEYS and all(np.isnan(v) for v in m.values())
    c = CASES["single5x7"]
    none = route.ssi_metrics(dev(np.zeros_like(c["gt"]))[None], dev(c["pred"])[None], MN, MX)[0].cpu().numpy()
    assert (none == 0).all()
    assert all(np.isnan(v) for v in M.compute_ssi_metrics_fused(dev(c["gt"]), dev(c["pred"]), **crop_args("single5x7")).values())


# ------------------------------------------------------------------------------------------------------------------ bit-exactness
def three_frames(name):
    """the case's frame under three different masks"""
    c = CASES[name]
    h, w = c["gt"].shape
    g = np.stack([c["gt"]] * 3)
    g[1, : h // 3] = 0.0
    g[1, :, w // 2:w // 2 + 3] = 20.0
    g[2, ::3, 1::2] = 0.0
    p = np.stack([c["pred"], c["pred"][::-1], c["pred"][:, ::-1]])
    return dev(g), dev(np.nan_to_num(p, nan=1.5))


@pytest.mark.parametrize("name", ["holes37x53", "big270x480"])
def test_frames_in_a_batch_equal_the_frames_alone(route, name):  # noqa: F811
    g, p = three_frames(name)
    out = route.ssi_metrics(g, p, MN, MX)
    assert tuple(out.shape) == (3, 41) and len({float(v) for v in out[:, 6]}) == 3
    for f in range(3):
        assert same_bits(route.ssi_metrics(g[f:f + 1], p[f:f + 1], MN, MX), out[f:f + 1]), (name, f)
    assert same_bits(route.ssi_metrics(g, p, MN, MX), out)


@pytest.mark.parametrize("pshape,name", [((19, 27), "holes37x53"), ((1, 1), "t5x7"), ((80, 96), "holes37x53"), ((135, 240), "big270x480")])
def test_resize_inside_the_kernels_equals_interpolate_then_score(route, pshape, name):  # noqa: F811
    c = CASES[name]
    g = dev(c["gt"])[None]
    rs = np.random.RandomState(pshape[0] * 1000 + pshape[1])
    small = dev((0.5 + 8.0 * rs.rand(1, *pshape)).astype(np.float32))
    up = F.interpolate(small[:, None], c["gt"].shape, mode="bilinear", align_corners=False)[:, 0].contiguous()
    crop = c["crop"]
    low = route.ssi_metrics(g, small, MN, MX, crop)
    assert same_bits(low, route.ssi_metrics(g, up, MN, MX, crop)), (pshape, name)
    assert low[0, 6] == c["n"] and bool(torch.isfinite(low).all())


def test_crop_limits_the_mask_and_the_pairs(route):  # noqa: F811
    from patchrefinerv2_amd import metrics as M
    c = CASES["garg37x53"]
    y0, y1, x0, x1 = c["crop"]
    cropped = score(route, "garg37x53")
    outside = c["gt"].copy()
    keep = np.zeros(outside.shape, bool)
    keep[y0:y1, x0:x1] = True
    outside[~keep] = 0.0  # the same pixel set without a crop: nothing outside is in the mask, no pair reaches across the border
    assert same_bits(route.ssi_metrics(dev(outside)[None], dev(c["pred"])[None], MN, MX), cropped)
    assert not same_bits(score(route, "holes37x53"), cropped)
    m = M.compute_ssi_metrics_fused(dev(c["gt"]), dev(c["pred"]), **crop_args("garg37x53"))
    close(m, c["want"], f"{route.DISPATCH} fused garg_crop")
    for crop in ((0, 37, 0, 0), (5, 5, 0, 53)):  # an empty crop: nothing is valid
        assert (route.ssi_metrics(dev(c["gt"])[None], dev(c["pred"])[None], MN, MX, crop).cpu().numpy() == 0).all()


def test_torch_op_and_c_abi_agree_bitwise(monkeypatch):
    from patchrefinerv2_amd import ops
    g, p = three_frames("big270x480")
    small = p[:, ::2, ::2].contiguous()
    got = {}
    for r in ("ctypes", "torch"):
        monkeypatch.setattr(ops, "DISPATCH", r)
        got[r] = (ops.ssi_metrics(g, p, MN, MX), ops.ssi_metrics(g, small, MN, MX, (30, 260, 10, 470)))
    assert same_bits(got["ctypes"][0], got["torch"][0]) and same_bits(got["ctypes"][1], got["torch"][1])


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_prediction_inside_the_mask(route, bad):  # noqa: F811
    from patchrefinerv2_amd import metrics as M
    c = CASES["holes37x53"]
    m = c["mask"]
    both = m[:-2, :-2] & m[2:, :-2] & m[:-2, 2:]  # a masked pixel that starts a vertical and a horizontal pair
    y, x = np.argwhere(both)[len(np.argwhere(both)) // 2]
    p = c["pred"].copy()
    p[y, x] = bad
    row = route.ssi_metrics(dev(c["gt"])[None], dev(p)[None], MN, MX)[0].cpu().numpy()
    assert row[6] == c["n"]  # N does not look at the prediction
    s = M.ssi_from_values(row)
    for k in ("ssi_l1", "ssi_gm", "gm", "ssi_gm_inv"):
        assert not np.isfinite(s[k]), (bad, k, s[k])
    p[y, x] = c["pred"][y, x]
    p[~m] = bad  # outside the mask nothing is looked at
    assert same_bits(route.ssi_metrics(dev(c["gt"])[None], dev(p)[None], MN, MX), score(route, "holes37x53"))


# ------------------------------------------------------------------------------------------------------------------ the datasets
def f64_bits(v):
    return struct.pack("<d", float(v))


def check_dataset(plain, ssi, **extra):
    """get_metrics with the flag: today's keys bit-equal to the run without it, then the new keys equal to the host restatement (on
    the prediction as the device resizes it)"""
    from patchrefinerv2_amd import metrics as M
    try:
        item = plain[0]
        gt = item["depth_gt"]
        assert gt.is_cuda and ssi[0]["depth_gt"].equal(gt)
        h, w = gt.shape[-2:]
        clean = torch.where((gt > plain.min_depth) & (gt < plain.max_depth), gt, torch.full_like(gt, 3.0))
        yy, xx = torch.meshgrid(torch.arange(h, device=DEV), torch.arange(w, device=DEV), indexing="ij")
        full = 0.6 * clean + 1.0 + 0.5 * torch.sin(xx / 3.0) * torch.cos(yy / 4.0)
        pred = F.interpolate(full, (h // 2 + 1, w // 2 + 3), mode="bilinear", align_corners=False)
        kw = dict(disp_gt_edges=item["boundary"], **{k: item[k] for k in extra})
        a, b = plain.get_metrics(gt, pred, **kw), ssi.get_metrics(gt, pred, **kw)
        assert tuple(b) == tuple(a) + SSI_KEYS and len(a) >= 10
        for k in a:
            assert f64_bits(a[k]) == f64_bits(b[k]), k
        up = F.interpolate(pred, (h, w), mode="bilinear", align_corners=False)
        want = M.compute_ssi_metrics(gt.cpu(), up.cpu(), garg_crop=False, eigen_crop=False, dataset="", min_depth_eval=plain.min_depth,
                                     max_depth_eval=plain.max_depth)
        assert np.isfinite(list(want.values())).all()
        close(b, want, type(plain).__name__)
        return a, b
    finally:
        for ds in (plain, ssi):
            if hasattr(ds, "close"):
                ds.close()


def test_image_dataset_get_metrics(tmp_path):
    img_dir, gt_dir, _ = write_general_tree(str(tmp_path), "eth3d", (37, 53), n=1)
    kw = dict(gt_format="eth3d", gt_shape=(37, 53), image_resolution=(37, 53), min_depth=MN, max_depth=MX)
    check_dataset(general_dataset(img_dir, gt_dir, **kw), general_dataset(img_dir, gt_dir, ssi_metrics=True, **kw))


def test_image_dataset_device_result_with_host_ground_truth(tmp_path):
    """no gt_format: the ground truth is a host tensor, the result is on the device -> still the fused route"""
    from patchrefinerv2_amd import metrics as M
    from patchrefinerv2_amd.tester import ImageDataset
    (tmp_path / "rgb").mkdir()
    c = CASES["holes37x53"]
    gt, pred = torch.from_numpy(np.nan_to_num(c["gt"]))[None, None], dev(np.nan_to_num(c["pred"], nan=2.0))[None, None]
    a = ImageDataset(str(tmp_path / "rgb"), min_depth=MN, max_depth=MX).get_metrics(gt, pred)
    b = ImageDataset(str(tmp_path / "rgb"), min_depth=MN, max_depth=MX, ssi_metrics=True).get_metrics(gt, pred)
    assert tuple(b) == tuple(a) + SSI_KEYS and all(f64_bits(a[k]) == f64_bits(b[k]) for k in a)
    close(b, M.compute_ssi_metrics(gt, pred.cpu(), **crop_args("holes37x53")), "ImageDataset (host gt)")


def test_u4k_dataset_get_metrics(tmp_path):
    root = str(tmp_path / "u4k")
    split = write_u4k_tree(root, [("00001", "00002", 1000.0, 0.5)], (38, 52))
    check_dataset(u4k_dataset(root, split, (38, 52)), u4k_dataset(root, split, (38, 52), ssi_metrics=True))


def test_eth_dataset_get_metrics_and_nanmean(tmp_path):
    split, _ = write_eth_tree(str(tmp_path), 1, (30, 44), (37, 53))
    a, b = check_dataset(eth_dataset(split, gt_shape=(37, 53)), eth_dataset(split, gt_shape=(37, 53), ssi_metrics=True), image_hr="image_hr")
    assert len(a) == 30
    ds = eth_dataset(split, gt_shape=(37, 53), ssi_metrics=True)
    nan_row = dict(b, **{k: float("nan") for k in SSI_KEYS})
    ev = ds.evaluate([b, nan_row])  # the nanmean: a frame without a fit does not poison the mean
    assert all(f64_bits(ev[k]) == f64_bits(b[k]) for k in SSI_KEYS)
