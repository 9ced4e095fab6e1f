"""GPU: ETHDataset -- csrc/evalgt.hip's edge-area kernels against the specification of tests/test_eth_dataset_host.py (exact: that file
asserts that no test image has a pixel near the threshold), csrc/gather.hip's image stage against its float32 restatement (bit for bit)
and torch's F.interpolate, and tester.ETHDataset through Tester.run and tools/test.py --test-type normal.  Both dispatch routes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_eth_dataset_host import (ETH_FRAMES, ETH_GT, ETH_PHOTO, ETH_RAW, ETH_SEED, FRACTION_CASES, KEYS, KEYS30, ONE_PIXEL_CASES,  # noqa: E402
                                   REGION_CASES, RESIZE_ATOL, RESIZE_CASES, dataset_image, edge_region_spec, edge_region_torch,
                                   eth_config_text, one_pixel_image, raw_depth, resize_source, scene, u8_resize_spec, u8_resize_torch,
                                   write_eth_tree)
from test_general_gt_host import bit_equal, decode_spec  # noqa: E402
from test_u4k_eval_gpu import OUT, PPS, SPLIT, _close, route  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------------------------ image_edge_region
@pytest.mark.parametrize("img_shape,gt_shape", REGION_CASES)
def test_edge_region_equals_the_spec_exactly(route, img_shape, gt_shape):
    img = scene(*img_shape)
    want = edge_region_spec(img, *gt_shape)
    got = route.image_edge_region(img.to(DEV), *gt_shape)
    assert got.dtype == torch.uint8 and tuple(got.shape) == gt_shape and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want), (img_shape, gt_shape, int((got.cpu().numpy() != want).sum()))
    assert torch.equal(route.image_edge_region(img.to(DEV), *gt_shape), got)  # the same bits on every call
    if min(img_shape) >= 12:
        assert 0 < want.mean() < 1
    # the reference's lines as torch ops on the same device (float32)
    assert torch.equal(edge_region_torch(img.to(DEV), *gt_shape), got.bool()), (img_shape, gt_shape)


def test_edge_region_routes_agree_bit_for_bit(monkeypatch):
    from patchrefinerv2_amd import ops
    img = scene(135, 240).to(DEV)
    out = []
    for r in ("ctypes", "torch"):
        monkeypatch.setattr(ops, "DISPATCH", r)
        out.append(ops.image_edge_region(img, 252, 448))
        out.append(ops.u8_image_resize(torch.from_numpy(resize_source((63, 95))).to(DEV), 34, 51))
    assert torch.equal(out[0], out[2]) and torch.equal(out[1], out[3])


@pytest.mark.parametrize("shape,gt_shape,y,x", ONE_PIXEL_CASES)
def test_edge_pixel_dilates_inside_the_frame_only(route, shape, gt_shape, y, x):
    img = one_pixel_image(shape, y, x)
    want = edge_region_spec(img, *gt_shape)
    got = route.image_edge_region(img.to(DEV), *gt_shape).cpu().numpy()
    assert np.array_equal(got, want) and 0 < want.mean() < 1, (shape, gt_shape, y, x)


def test_other_fractions_and_wrong_inputs(route):
    img = scene(37, 53)
    for frac in FRACTION_CASES + (0.0,):  # (0: every pixel)
        want = edge_region_spec(img, 70, 99, frac)
        assert np.array_equal(route.image_edge_region(img.to(DEV), 70, 99, frac).cpu().numpy(), want) and want.any(), frac
    with pytest.raises(ValueError, match="GPU"):
        route.image_edge_region(img, 70, 99)
    with pytest.raises(ValueError, match="shape"):
        route.image_edge_region(torch.zeros(1, 4, 4, device=DEV), 8, 8)


def test_constant_image_is_all_edge_and_noedge_is_nan(route):
    from patchrefinerv2_amd import tester
    img = torch.full((3, 24, 40), 0.25, device=DEV)
    region = route.image_edge_region(img, 37, 53)
    assert region.all() and tuple(region.shape) == (37, 53)
    ds = tester.ETHDataset.__new__(tester.ETHDataset)
    ds.min_depth, ds.max_depth = 1e-3, 80
    gt, boundary = decode_spec("eth3d", raw_depth((37, 53), 2))
    ratio = 1.05 + 0.2 * np.random.RandomState(0).rand(37, 53)
    pred = torch.from_numpy((np.where(gt > 0, gt, 1.0) * ratio).astype(np.float32))[None, None].to(DEV)
    m = ds.get_metrics(torch.from_numpy(gt)[None, None].to(DEV), pred, torch.from_numpy(boundary).to(DEV), image_hr=img)
    assert tuple(m) == KEYS30
    for k in KEYS:
        assert (m["noedge_" + k] == 0.0) if k == "see" else np.isnan(m["noedge_" + k]), k  # an empty set: NaN means, see 0 (metric.py:139-147)
        assert m["edge_" + k] == m[k] and not np.isnan(m[k]), k
    with pytest.raises(ValueError, match="image_hr"):
        ds.get_metrics(torch.from_numpy(gt)[None, None].to(DEV), pred, torch.from_numpy(boundary).to(DEV))


# ------------------------------------------------------------------------------------------------------------------ u8_image_resize
@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_u8_image_resize(route, src, dst):
    """bit-equal to the float32 restatement of include/prv2.h; against F.interpolate within RESIZE_ATOL: torch's own kernels (CPU and
    device) contract their multiply-adds, this one does not -- four times the largest difference measured against torch's CPU on
    these shapes (tests/test_eth_dataset_host.py RESIZE_MEASURED_MAX_ABS)"""
    x = resize_source(src)
    xd = torch.from_numpy(x).to(DEV)
    got = route.u8_image_resize(xd, *dst)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3,) + dst and got.is_contiguous()
    assert torch.equal(got.cpu(), torch.from_numpy(u8_resize_spec(x, *dst))), (src, dst)
    ref_cpu = torch.from_numpy(u8_resize_torch(x, *dst))
    ref_dev = F.interpolate(xd.permute(2, 0, 1)[None].float() / 255, dst, mode="bilinear", align_corners=True)[0]
    d_cpu, d_dev = float((got.cpu() - ref_cpu).abs().max()), float((got - ref_dev).abs().max())
    print(f"{src}->{dst}: max |kernel - torch CPU| = {d_cpu:.3e}, max |kernel - torch device| = {d_dev:.3e}")
    assert d_cpu <= RESIZE_ATOL and d_dev <= RESIZE_ATOL, (src, dst, d_cpu, d_dev)
    if src == dst:  # identity: u8_image's bits, and torch's
        assert torch.equal(got, route.u8_image(xd, swap_rb=False)) and torch.equal(got.cpu(), ref_cpu)
    assert torch.equal(route.u8_image_resize(xd, *dst), got)


def test_u8_image_resize_rejects_wrong_inputs(route):
    with pytest.raises(ValueError, match="GPU"):
        route.u8_image_resize(torch.zeros(4, 4, 3, dtype=torch.uint8), 8, 8)
    with pytest.raises(ValueError, match="GPU uint8"):
        route.u8_image_resize(torch.zeros(4, 4, 3, device=DEV), 8, 8)
    with pytest.raises(ValueError, match="size"):
        route.u8_image_resize(torch.zeros(4, 4, 3, dtype=torch.uint8, device=DEV), 0, 8)


# ------------------------------------------------------------------------------------------------------------------ dataset and CLI
def _model_lines():
    return (f"model = dict(config=dict(patch_process_shape={list(PPS)}, image_raw_shape={list(ETH_RAW)}, patch_split_num={list(SPLIT)},\n"
            "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")


@pytest.fixture(scope="module")
def eth_run(tmp_path_factory):
    """a two-frame synthetic ETH3D tree (PNG photographs, raw float32 ground truth of another aspect holding NaN / inf / 0), the model
    the CLI would build for it (synthetic weights), and one Tester.run; ``scored`` records what get_metrics was handed"""
    from patchrefinerv2_amd import models, weights as W  # noqa: F401
    from patchrefinerv2_amd.registry import DATASETS, Config, build_model
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    tmp = tmp_path_factory.mktemp("eth")
    split, items = write_eth_tree(str(tmp / "data"), ETH_FRAMES, ETH_PHOTO, ETH_GT, seed=ETH_SEED)
    cfg_path = tmp / "cfg.py"
    cfg_path.write_text(eth_config_text(split, ETH_GT, ETH_RAW, extra=_model_lines()))
    cfg = Config.fromfile(str(cfg_path))
    mcfg = cfg.model.to_dict()
    mcfg["config"].update(prec="bf16x3", max_batch=41, n_streams=3)  # tools/test.py's defaults
    model = build_model(mcfg)
    model.load_state_dict(W.synth_state_dict(model.spec(), seed=0), strict=True)
    ds = DATASETS.build(cfg.val_dataloader.dataset.to_dict())
    fetched = [ds[i] for i in (0, 1, 0)]  # in order (the read one ahead is used) and back (it is dropped)
    scored = []
    own = ds.get_metrics

    def recording(depth_gt, result, disp_gt_edges=None, **kw):
        scored.append((depth_gt.cpu(), result.cpu(), disp_gt_edges.cpu(), kw["image_hr"].cpu()))
        return own(depth_gt, result, disp_gt_edges=disp_gt_edges, **kw)
    ds.get_metrics = recording
    t = Tester(None, RunnerInfo(), ds, model)
    one = t.run(cai_mode="m1", image_raw_shape=ETH_RAW, patch_split_num=SPLIT, seed=621, frame_batch=1)
    ds.close()
    return dict(tmp=tmp, cfg=str(cfg_path), ds=ds, items=items, fetched=fetched, one=one, scored=scored, last_eval=dict(t.last_eval))


def test_dataset_items_equal_the_spec(eth_run):
    ds, items = eth_run["ds"], eth_run["items"]
    assert len(ds) == ETH_FRAMES and [i["img_path"] for i in ds.data_infos] == [it["img"] for it in items]
    for idx, item in zip((0, 1, 0), eth_run["fetched"]):
        it = items[idx]
        assert set(item) == {"image_hr", "depth_gt", "boundary", "img_file_basename"}
        assert item["img_file_basename"] == os.path.splitext(it["img"])[0].replace("/", "_")[1:]
        assert item["image_hr"].is_cuda and tuple(item["image_hr"].shape) == (3,) + ETH_RAW
        assert torch.equal(item["image_hr"].cpu(), dataset_image(idx)), idx  # PNG decode -> bytes / 255 -> bilinear, bit for bit
        want_d, want_b = decode_spec("eth3d", it["depth"])
        assert tuple(item["depth_gt"].shape) == (1, 1) + ETH_GT and item["boundary"].dtype == torch.uint8
        assert bit_equal(item["depth_gt"][0, 0].cpu().numpy(), want_d) and np.array_equal(item["boundary"].cpu().numpy(), want_b)
        assert want_b.sum() > 50 and not np.isfinite(it["depth"]).all() and (want_d == 0).any()


def test_dataset_without_input_size_shallow_is_u8_image(eth_run):
    from patchrefinerv2_amd import tester
    ds = tester.ETHDataset("infer", eth_run["ds"].split, dict(input_size_deep=[448, 448]), 1e-3, 80, gt_shape=ETH_GT)
    try:
        item = ds[1]
    finally:
        ds.close()
    want = eth_run["items"][1]["pixels"].astype(np.float32) / np.float32(255.0)
    assert torch.equal(item["image_hr"].cpu(), torch.from_numpy(np.ascontiguousarray(want.transpose(2, 0, 1))))
    bad = tester.ETHDataset("infer", eth_run["ds"].split, dict(input_size_deep=[448, 448]), 1e-3, 80, gt_shape=(ETH_GT[0] + 1, ETH_GT[1]))
    try:
        with pytest.raises(ValueError, match=re.escape(eth_run["items"][0]["gt"])):
            bad[0]
    finally:
        bad.close()


def test_get_metrics_equals_three_host_compute_metrics_calls(eth_run):
    """eth_dataset.py:277-289 on the host with the specification's mask, against the one fused pass of Tester.run"""
    from patchrefinerv2_amd import metrics as M
    one = eth_run["one"]
    assert [r["name"] for r in one] == [i["img_file_basename"] for i in eth_run["ds"].data_infos] and len(eth_run["scored"]) == ETH_FRAMES
    for idx, (r, (gt, result, edges, image)) in enumerate(zip(one, eth_run["scored"])):
        assert r["shape"] == (1, 1) + OUT == tuple(result.shape) and tuple(gt.shape) == (1, 1) + ETH_GT  # scoring resizes the map
        assert torch.equal(image, dataset_image(idx))
        mask = torch.from_numpy(edge_region_spec(image, *ETH_GT).astype(bool))
        assert 0 < float(mask.float().mean()) < 0.5
        kw = dict(disp_gt_edges=edges.numpy(), min_depth_eval=1e-3, max_depth_eval=80, garg_crop=False, eigen_crop=False, dataset="")
        with np.errstate(invalid="ignore"):
            parts = [("edge_", M.compute_metrics(gt, result.clone(), additional_mask=mask, **kw)),
                     ("noedge_", M.compute_metrics(gt, result.clone(), additional_mask=~mask, **kw)),
                     ("", M.compute_metrics(gt, result.clone(), **kw))]
        ref = {pre + k: v for pre, m in parts for k, v in m.items()}
        assert tuple(r["metrics"]) == tuple(ref) == KEYS30
        _close(r["metrics"], ref, r["name"])
        assert r["metrics"]["see"] > 0 and r["metrics"]["edge_a1"] != r["metrics"]["noedge_a1"] and 0 < r["metrics"]["abs_rel"] < 100
    assert one[0]["metrics"] != one[1]["metrics"]


def test_last_eval_is_the_nanmean(eth_run):
    one, ev = eth_run["one"], eth_run["last_eval"]
    assert tuple(ev) == KEYS30
    for k in KEYS30:
        assert ev[k] == float(np.nanmean([r["metrics"][k] for r in one])), k


def test_cli_test_type_normal_prints_the_thirty_keys(eth_run):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), eth_run["cfg"], "--synthetic-weights", "--cai-mode", "m1",
                        "--test-type", "normal", "--image-raw-shape", str(ETH_RAW[0]), str(ETH_RAW[1]), "--patch-split-num", "2", "2"],
                       capture_output=True, text=True, timeout=600, cwd=str(eth_run["tmp"]))
    assert r.returncode == 0, r.stderr[-2000:]

    def parse(text):
        return {k: float(v) for k, v in (kv.split(" ") for kv in text.split(", "))}
    for res in eth_run["one"]:
        assert f"{res['name']}: depth {(1, 1) + OUT}" in r.stdout
        line = re.search(rf"{res['name']}: (edge_a1 .*)", r.stdout)
        assert line, r.stdout[-2000:]
        printed = parse(line.group(1))
        assert tuple(printed) == KEYS30
        for k, v in printed.items():
            assert abs(v - res["metrics"][k]) <= 1e-6 * max(1.0, abs(res["metrics"][k])), (k, v, res["metrics"][k])
    summary = [ln for ln in r.stdout.splitlines() if ln.startswith("[rank 0] edge_a1 ")]
    assert len(summary) == 1, r.stdout[-2000:]
    printed = parse(summary[0][len("[rank 0] "):])
    assert tuple(printed) == KEYS30
    for k, v in printed.items():
        assert abs(v - eth_run["last_eval"][k]) <= 1e-4 * max(1.0, abs(eth_run["last_eval"][k])), (k, v)
