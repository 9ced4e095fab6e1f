"""GPU: the U4K dataset evaluation -- csrc/evalgt.hip's three kernels against numpy (both dispatch routes), compute_metrics_fused
against the pinned host metrics and the reference's recorded outputs, and Tester.run / tools/test.py --test-type normal over a
synthetic U4K tree."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_u4k_eval_host import write_u4k_tree  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
torch.set_grad_enabled(False)
SHAPES = [(1, 1), (2, 3), (37, 53), (5, 1), (270, 480)]  # one pixel; tiny; no multiple of 4 or 64; one column; float4 rows, many blocks
MN, MX = 0.1, 10.0


@pytest.fixture(params=["ctypes", "torch"])
def route(request, monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    monkeypatch.setattr(ops, "DISPATCH", request.param)
    return ops


# ------------------------------------------------------------------------------------------------------------------ u8_image
@pytest.mark.parametrize("shape", SHAPES)
def test_u8_image_is_bit_equal_to_numpy(route, shape):
    img = np.random.RandomState(shape[0] * 1000 + shape[1]).randint(0, 256, shape + (3,)).astype(np.uint8)
    if img.size >= 768:
        img.reshape(-1)[:256] = np.arange(256)  # every byte value
    for swap in (True, False):
        want = img.astype(np.float32)[:, :, ::-1].copy() / 255.0 if swap else img.astype(np.float32) / 255.0
        got = route.u8_image(torch.from_numpy(img).to(DEV), swap_rb=swap)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3,) + shape
        assert torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(want.transpose(2, 0, 1)))), (shape, swap)


# ------------------------------------------------------------------------------------------------------------------ disp_gt
def _disp(shape, seed):
    """smooth disparity with unit-plus steps on every frame border and in every corner, a zero and a NaN"""
    h, w = shape
    rs = np.random.RandomState(seed)
    d = (5.0 + 0.3 * rs.rand(h, w)).astype(np.float32)
    d[0, ::2] += 3.0
    d[-1, 1::2] += 3.0
    d[::2, 0] += 3.0
    d[1::2, -1] += 3.0
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        d[y, x] += 7.0
    if h * w > 6:
        d[h // 2, w // 2] = 0.0
        d[h // 3, w // 3] = np.nan
        d[(2 * h) // 3, w // 4] += 1.0000001  # just over / at the threshold
    return d


@pytest.mark.parametrize("shape", SHAPES)
def test_disp_gt_depth_and_boundary(route, shape):
    from patchrefinerv2_amd import metrics as M
    d = _disp(shape, 7)
    factor = 123.456
    depth, boundary = route.disp_gt(torch.from_numpy(d).to(DEV), factor, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.float32(factor) / d
        edges = M.get_boundaries(d, th=1.0, dilation=0)
    assert depth.dtype == torch.float32 and boundary.dtype == torch.uint8
    got = depth.cpu().numpy()
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if d.size > 6:
        assert np.isinf(got[shape[0] // 2, shape[1] // 2]) and np.isnan(got[shape[0] // 3, shape[1] // 3])
    assert np.array_equal(boundary.cpu().numpy(), edges.astype(np.uint8)), shape
    if min(shape) > 1:
        assert boundary[0, 0] and boundary[0, -1] and boundary[-1, 0] and boundary[-1, -1]


# ------------------------------------------------------------------------------------------------------------------ depth_metrics
def ref_sums(gt, pred, boundary=None, region=None, mn=MN, mx=MX, crop=None):
    """float64 numpy recomputation of prv2_depth_metrics for ONE frame -> (sums [S, 12], sums of |term| [S, 12])"""
    from patchrefinerv2_amd import metrics as M
    h, w = gt.shape
    mn32, mx32 = np.float32(mn), np.float32(mx)
    p = pred.astype(np.float32).copy()
    with np.errstate(invalid="ignore"):
        p[np.isnan(p)] = mn32
        p[p < mn32] = mn32
        p[p > mx32] = mx32
        valid = (gt > mn32) & (gt < mx32)
    if crop is not None:
        m = np.zeros((h, w), bool)
        m[crop[0]:crop[1], crop[2]:crop[3]] = True
        valid &= m
    with np.errstate(invalid="ignore"):
        see_map = M.soft_edge_error(p, gt, radius=1)  # fp32
    sets = [valid] if region is None else [valid, valid & (region != 0), valid & (region == 0)]
    out, mag = [], []
    for v in sets:
        g64, p64 = gt[v].astype(np.float64), p[v].astype(np.float64)
        ratio = np.maximum(g64 / p64, p64 / g64)
        d = g64 - p64
        err = np.log(p64) - np.log(g64)
        terms = [np.ones_like(d), ratio < 1.25, ratio < 1.25 ** 2, ratio < 1.25 ** 3, np.abs(d) / g64, d * d,
                 np.abs(np.log10(g64) - np.log10(p64)), err * err, err, d * d / g64]
        e = v & (boundary != 0) if boundary is not None else np.zeros_like(v)
        terms += [np.ones(int(e.sum())), see_map[e].astype(np.float64)]
        out.append([float(np.sum(np.asarray(t, np.float64))) for t in terms])
        mag.append([float(np.sum(np.abs(np.asarray(t, np.float64)))) for t in terms])
    return np.array(out), np.array(mag)


def check_sums(got, want, mag, tag=""):
    """counts exactly; every sum within 1e-9 * sum |term| (2^-53 * N for N <= 2^23 terms plus a few ulp of the device's log)"""
    assert got.shape == want.shape, (got.shape, want.shape)
    for s in range(want.shape[0]):
        for k in (0, 1, 2, 3, 10):
            assert got[s, k] == want[s, k], (tag, s, k, got[s, k], want[s, k])
        for k in (4, 5, 6, 7, 8, 9, 11):
            if np.isnan(want[s, k]) or np.isinf(want[s, k]):
                assert str(got[s, k]) == str(want[s, k]), (tag, s, k, got[s, k], want[s, k])
            else:
                assert abs(got[s, k] - want[s, k]) <= 1e-9 * mag[s, k], (tag, s, k, got[s, k], want[s, k], mag[s, k])


def _frame(shape, seed, hard=True):
    """gt, pred, boundary, region of one frame: gt with invalid (zero, too far, inf) pixels, pred with NaN / +inf / negative / out-of-range
    pixels, boundary pixels on every frame edge and corner"""
    from patchrefinerv2_amd import metrics as M
    h, w = shape
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    gt = (1.0 + 4.0 * (x > w * 0.45) + 2.0 * (y > h * 0.5) + 0.5 * rs.rand(h, w)).astype(np.float32)
    pred = (gt * (0.7 + 0.6 * rs.rand(h, w))).astype(np.float32)
    if hard and h * w > 6:
        idx = rs.permutation(h * w)
        n = max(1, h * w // 50)
        pf, gf = pred.reshape(-1), gt.reshape(-1)
        pf[idx[:n]] = np.nan
        pf[idx[n:2 * n]] = np.inf
        pf[idx[2 * n:3 * n]] = -3.0
        pf[idx[3 * n:4 * n]] = 50.0
        pf[idx[4 * n:5 * n]] = 0.01
        gf[idx[5 * n:6 * n]] = 0.0
        gf[idx[6 * n:7 * n]] = 30.0
        gf[idx[7 * n:8 * n]] = np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        boundary = M.get_boundaries(np.float32(40.0) / gt, th=1.0, dilation=0).astype(np.uint8)
    boundary[0, :] = boundary[-1, :] = 1
    boundary[:, 0] = boundary[:, -1] = 1
    region = (rs.rand(h, w) < 0.4).astype(np.uint8)
    return gt, pred, boundary, region


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("with_region", [False, True])
def test_depth_metrics_against_float64_numpy(route, shape, with_region):
    gt, pred, boundary, region = _frame(shape, 11 + shape[0])
    region = region if with_region else None
    g, p, b, r = _dev(gt, pred, boundary, region)
    got = route.depth_metrics(g, p, b, r, MN, MX)
    assert got.dtype == torch.float64 and tuple(got.shape) == (1, 3 if with_region else 1, 12)
    want, mag = ref_sums(gt, pred, boundary, region)
    check_sums(got[0].cpu().numpy(), want, mag, shape)
    assert torch.equal(route.depth_metrics(g, p, b, r, MN, MX), got)  # bit-identical from call to call
    if shape == (270, 480):
        assert want[0, 0] > 1e5 and want[0, 10] > 1000  # the case is not vacuous
    # without a boundary map the soft-edge sums are zero and the rest is unchanged
    nb = route.depth_metrics(g, p, None, r, MN, MX)[0].cpu().numpy()
    assert np.array_equal(nb[:, :10], got[0].cpu().numpy()[:, :10], equal_nan=True) and not nb[:, 10:].any()


@pytest.mark.parametrize("shape,crop", [((37, 53), (5, 30, 7, 41)), ((270, 480), (110, 267, 17, 462)), ((270, 480), (0, 270, 4, 8)),
                                        ((37, 53), (10, 10, 0, 53)), ((2, 3), (1, 2, 1, 3))])
def test_depth_metrics_crop_rectangle(route, shape, crop):
    gt, pred, boundary, region = _frame(shape, 23)
    got = route.depth_metrics(*_dev(gt, pred, boundary, region), MN, MX, crop=crop)[0].cpu().numpy()
    want, mag = ref_sums(gt, pred, boundary, region, crop=crop)
    check_sums(got, want, mag, (shape, crop))


def test_depth_metrics_all_invalid_frame_and_two_frames(route):
    """B = 2 with different frames (one of them without a valid pixel): each row is its own frame's sums; the empty frame gives NaN
    metrics and see = 0"""
    from patchrefinerv2_amd import metrics as M
    shape = (37, 53)
    g0, p0, b0, r0 = _frame(shape, 31)
    g1, p1, b1, r1 = _frame(shape, 32)
    g1[:] = 0.0  # nothing valid
    gt, pred, bnd, reg = np.stack([g0, g1]), np.stack([p0, p1]), np.stack([b0, b1]), np.stack([r0, r1])
    got = route.depth_metrics(*_dev(gt, pred, bnd, reg), MN, MX)
    assert tuple(got.shape) == (2, 3, 12)
    assert torch.equal(route.depth_metrics(*_dev(gt, pred, bnd, reg), MN, MX), got)
    for f, (g, p, b, r) in enumerate(((g0, p0, b0, r0), (g1, p1, b1, r1))):
        want, mag = ref_sums(g, p, b, r)
        check_sums(got[f].cpu().numpy(), want, mag, f)
        one = route.depth_metrics(*_dev(g, p, b, r), MN, MX)
        assert torch.equal(one[0], got[f])  # a frame's sums do not depend on its batch
    assert not got[1].any()
    rows = M.compute_metrics_fused(torch.from_numpy(gt)[:, None], torch.from_numpy(pred)[:, None].to(DEV), garg_crop=False, eigen_crop=False,
                                   min_depth_eval=MN, max_depth_eval=MX, disp_gt_edges=torch.from_numpy(bnd))
    assert isinstance(rows, list) and len(rows) == 2
    assert rows[1]["see"] == 0.0 and all(np.isnan(v) for k, v in rows[1].items() if k != "see")
    assert not any(np.isnan(v) for v in rows[0].values())


def test_depth_metrics_swapped_frames_differ(route):
    """the frame index reaches the maps: B = 2 in the other order gives the rows in the other order"""
    a, b = _frame((270, 480), 41), _frame((270, 480), 42)
    ab = route.depth_metrics(*_dev(*(np.stack(t) for t in zip(a, b))), MN, MX)
    ba = route.depth_metrics(*_dev(*(np.stack(t) for t in zip(b, a))), MN, MX)
    assert torch.equal(ab[0], ba[1]) and torch.equal(ab[1], ba[0]) and not torch.equal(ab[0], ab[1])


# ------------------------------------------------------------------------------------------------------------------ compute_metrics_fused
def _close(got, ref, tag=""):
    """the project's tolerance for device metrics against the pinned host ones (tests/test_host_logic.py:173)"""
    assert set(got) == set(ref), (tag, set(got) ^ set(ref))
    for k in ref:
        np.testing.assert_allclose(float(got[k]), float(ref[k]), rtol=2e-5, atol=1e-7, err_msg=f"{tag} {k}")


def test_fused_matches_the_reference_outputs():
    """tests/golden/output_stage.npz: the reference's own compute_metrics results (m1: u4k protocol with edges; m2: garg crop, resized
    low-resolution prediction)"""
    from patchrefinerv2_amd import metrics as M
    z = np.load(os.path.join(ROOT, "tests", "golden", "output_stage.npz"))
    gt, pred, pred_lo, edges = (torch.from_numpy(z[k]) for k in ("gt", "pred", "pred_lo", "edges"))
    m1 = M.compute_metrics_fused(gt, pred.clone().to(DEV), garg_crop=False, eigen_crop=False, dataset="u4k", min_depth_eval=0.1, max_depth_eval=10,
                                 disp_gt_edges=edges)
    m2 = M.compute_metrics_fused(gt.to(DEV), pred_lo.clone().to(DEV), garg_crop=True, eigen_crop=False, dataset="kitti", min_depth_eval=0.1,
                                 max_depth_eval=10)
    for tag, m in (("m1", m1), ("m2", m2)):
        keys = {k[len(tag) + 1:] for k in z.files if k.startswith(tag + "_")}
        assert set(m) == keys, (tag, set(m) ^ keys)
        for k, v in m.items():
            np.testing.assert_allclose(v, float(z[f"{tag}_{k}"]), rtol=2e-5, atol=1e-7, err_msg=f"{tag} {k}")


@pytest.mark.parametrize("shape", [(37, 53), (270, 480)])
def test_fused_matches_host_compute_metrics_and_three_sets(shape):
    from patchrefinerv2_amd import metrics as M
    gt, pred, boundary, region = _frame(shape, 51, hard=False)
    pred[3, 5], pred[4, 6], pred[5, 7] = np.nan, np.inf, -1.0
    gt[6, 8] = 0.0
    tg, tp = torch.from_numpy(gt)[None, None], torch.from_numpy(pred)[None, None]
    te, tr = torch.from_numpy(boundary.astype(np.float32)), torch.from_numpy(region.astype(bool))
    kw = dict(garg_crop=False, eigen_crop=False, dataset="", min_depth_eval=MN, max_depth_eval=MX)
    for crops in (kw, dict(kw, garg_crop=True), dict(kw, eigen_crop=True, dataset="kitti"), dict(kw, eigen_crop=True, dataset="nyu")):
        _close(M.compute_metrics_fused(tg, tp.to(DEV), disp_gt_edges=te, **crops), M.compute_metrics(tg, tp.clone(), disp_gt_edges=te, **crops),
               str(crops))
    _close(M.compute_metrics_fused(tg, tp.to(DEV), **kw), M.compute_metrics(tg, tp.clone(), **kw), "no edges")
    # one call with a region == three calls with additional_mask none / region / ~region, bit for bit
    three = M.compute_metrics_fused(tg, tp.to(DEV), disp_gt_edges=te, region=tr, **kw)
    parts = [("", None), ("edge_", tr), ("noedge_", ~tr)]
    assert set(three) == {pre + k for pre, _ in parts for k in ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel", "see")}
    for pre, mask in parts:
        one = M.compute_metrics_fused(tg, tp.to(DEV), disp_gt_edges=te, additional_mask=mask, **kw)
        assert {pre + k: v for k, v in one.items()} == {k: v for k, v in three.items() if (k.startswith(pre) if pre else "edge_" not in k)}
        _close(one, M.compute_metrics(tg, tp.clone(), disp_gt_edges=te, additional_mask=mask, **kw), pre)
    # a low-resolution prediction is resized first, like the existing functions
    lo = torch.from_numpy(np.ascontiguousarray(_frame(shape, 52, hard=False)[1][::2, ::2]))[None, None]
    if min(lo.shape[-2:]) > 1:
        _close(M.compute_metrics_fused(tg, lo.to(DEV), disp_gt_edges=te, **kw), M.compute_metrics(tg, lo.clone(), disp_gt_edges=te, **kw), "resized")


# ------------------------------------------------------------------------------------------------------------------ end to end
RAW, SPLIT, PPS = (256, 512), (2, 2), (112, 224)  # oracle.cases.E2E_V2: the smallest V2 case the end-to-end GPU tests use
OUT = (SPLIT[0] * PPS[0], SPLIT[1] * PPS[1])  # the model's map: split x patch_process_shape, smaller than the frame -- scoring resizes it
FRAMES = [("00001", "00004", 480.0, 0.35), ("00001", "00002", 512.0, 0.3)]


def _write_cfg(tmp_path, root):
    cfg = tmp_path / "cfg.py"
    cfg.write_text(f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n"
                   f"model = dict(config=dict(patch_process_shape={list(PPS)}, image_raw_shape={list(RAW)}, patch_split_num={list(SPLIT)},\n"
                   "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n"
                   f"val_dataloader = dict(dataset=dict(data_root={root!r}, split={os.path.join(root, 'splits', 'val.txt')!r}))\n")
    return str(cfg)


@pytest.fixture(scope="module")
def u4k_run(tmp_path_factory):
    """a two-frame synthetic U4K tree, the model the CLI would build for it (synthetic weights), and Tester.run with one and two
    frames per call; ``scored`` records what get_metrics was handed"""
    from patchrefinerv2_amd import models, weights as W  # noqa: F401
    from patchrefinerv2_amd.registry import DATASETS, Config, build_model
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    tmp = tmp_path_factory.mktemp("u4k")
    root = str(tmp / "data")
    write_u4k_tree(root, FRAMES, RAW, seed=5)
    cfg_path = _write_cfg(tmp, root)
    cfg = Config.fromfile(cfg_path)
    mcfg = cfg.model.to_dict()
    mcfg["config"].update(prec="bf16x3", max_batch=41, n_streams=3)  # tools/test.py's defaults
    model = build_model(mcfg)
    model.load_state_dict(W.synth_state_dict(model.spec(), seed=0), strict=True)
    ds = DATASETS.build(dict(cfg.val_dataloader.dataset.to_dict(), image_raw_shape=list(RAW)))
    scored = []
    fused = ds.get_metrics

    def recording(depth_gt, result, disp_gt_edges=None, **kw):
        scored.append((depth_gt.cpu(), result.cpu(), disp_gt_edges.cpu()))
        return fused(depth_gt, result, disp_gt_edges=disp_gt_edges, **kw)
    ds.get_metrics = recording
    t = Tester(None, RunnerInfo(), ds, model)
    one = t.run(cai_mode="m1", image_raw_shape=RAW, patch_split_num=SPLIT, seed=621, frame_batch=1)
    last_eval = dict(t.last_eval)
    n_one = len(scored)
    two = t.run(cai_mode="m1", image_raw_shape=RAW, patch_split_num=SPLIT, seed=621, frame_batch=2)
    item = ds[1]
    ds.close()
    return dict(tmp=tmp, root=root, cfg=cfg_path, ds=ds, one=one, two=two, scored=scored[:n_one], last_eval=last_eval, item=item)


def test_dataset_items_are_the_host_decode(u4k_run):
    from patchrefinerv2_amd import metrics as M
    ds, item = u4k_run["ds"], u4k_run["item"]
    info = ds.data_infos[1]
    assert [i["img_file_basename"] for i in ds.data_infos] == ["0001_Image0_00002", "0001_Image0_00004"]
    assert item["img_file_basename"] == info["img_file_basename"] == "0001_Image0_00004"
    image = np.fromfile(info["img_path"], dtype=np.uint8).reshape(*RAW, 3)
    image = image.astype(np.float32)[:, :, ::-1].copy() / 255.0
    assert item["image_hr"].is_cuda and torch.equal(item["image_hr"].cpu(), torch.from_numpy(image.transpose(2, 0, 1).copy()))
    disp = np.load(info["depth_map_path"]).astype(np.float32)
    with np.errstate(divide="ignore"):
        depth = np.float32(info["depth_factor"]) / disp
    assert tuple(item["depth_gt"].shape) == (1, 1) + RAW and torch.equal(item["depth_gt"].cpu()[0, 0], torch.from_numpy(depth))
    assert np.array_equal(item["boundary"].cpu().numpy(), M.get_boundaries(disp, th=1, dilation=0).astype(np.uint8))
    assert item["boundary"].sum() > 100


def test_tester_run_metrics_equal_host_compute_metrics(u4k_run):
    from patchrefinerv2_amd import metrics as M
    ds, one = u4k_run["ds"], u4k_run["one"]
    assert [r["name"] for r in one] == ["0001_Image0_00002", "0001_Image0_00004"] and len(u4k_run["scored"]) == 2
    for r, info, (gt, result, edges) in zip(one, ds.data_infos, u4k_run["scored"]):
        assert r["shape"] == (1, 1) + OUT == tuple(result.shape) and tuple(gt.shape) == (1, 1) + RAW
        disp = np.load(info["depth_map_path"]).astype(np.float32)
        with np.errstate(divide="ignore"):
            assert torch.equal(gt[0, 0], torch.from_numpy(np.float32(info["depth_factor"]) / disp))
        ref = M.compute_metrics(gt, result, disp_gt_edges=M.get_boundaries(disp, th=1, dilation=0), min_depth_eval=1e-3, max_depth_eval=80,
                                garg_crop=False, eigen_crop=False, dataset="")
        _close(r["metrics"], ref, r["name"])
        assert r["metrics"]["see"] > 0 and 0 < r["metrics"]["abs_rel"] < 100
    assert one[0]["metrics"] != one[1]["metrics"]
    ev = u4k_run["last_eval"]
    assert "see" in ev and ev["see"] == float(np.mean([r["metrics"]["see"] for r in one]))
    assert set(ev) == set(one[0]["metrics"])


def test_frame_batch_two_gives_the_same_dicts(u4k_run):
    assert [r["metrics"] for r in u4k_run["two"]] == [r["metrics"] for r in u4k_run["one"]]
    assert [r["name"] for r in u4k_run["two"]] == [r["name"] for r in u4k_run["one"]]


def test_cli_test_type_normal_prints_the_metrics(u4k_run):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), u4k_run["cfg"], "--synthetic-weights", "--cai-mode", "m1",
                        "--test-type", "normal", "--image-raw-shape", str(RAW[0]), str(RAW[1]), "--patch-split-num", "2", "2"],
                       capture_output=True, text=True, timeout=600, cwd=str(u4k_run["tmp"]))
    assert r.returncode == 0, r.stderr[-2000:]
    for res in u4k_run["one"]:
        assert f"{res['name']}: depth {(1, 1) + OUT}" in r.stdout
        line = re.search(rf"{res['name']}: (a1 .*)", r.stdout)
        assert line, r.stdout[-2000:]
        printed = {k: float(v) for k, v in (kv.split(" ") for kv in line.group(1).split(", "))}
        assert set(printed) == set(res["metrics"])
        for k, v in printed.items():
            assert abs(v - res["metrics"][k]) <= 1e-6 * max(1.0, abs(res["metrics"][k])), (k, v, res["metrics"][k])
    summary = [ln for ln in r.stdout.splitlines() if " see " in ln and "abs_rel" in ln and "Image0" not in ln]
    assert summary, r.stdout[-2000:]
