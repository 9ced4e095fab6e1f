"""GPU: CityScapesDataset -- csrc/evalgt.hip's ground-truth decode and pixel-set kernels and csrc/edges.hip's segmentation-edge detector
against the specification of tests/test_cityscapes_host.py (depth bit for bit, every mask pixel for pixel), and the dataset through
Tester.run and tools/test.py --test-type cityscapes over a synthetic tree.  Both dispatch routes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_cityscapes_host import (CS_FRAMES, CS_SEED, CS_SHAPE, KEYS17, cityscapes_config_text, cli_dataset, cs_factor, decode_spec_cs, disp_scene,  # noqa: E402
                                  masks_spec, seg_canny_spec, seg_scene, write_cityscapes_tree)
from test_eth_dataset_host import edge_region_spec  # noqa: E402
from test_general_gt_host import bit_equal  # noqa: E402
from test_u4k_eval_gpu import PPS, SPLIT, _close, route  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
torch.set_grad_enabled(False)
OUT = (SPLIT[0] * PPS[0], SPLIT[1] * PPS[1])  # the model's map: larger than the 64 x 128 ground truth -- scoring resizes it
# (3, 3), (8, 16), (37, 53): the scalar tails; (64, 128): the vector path; (135, 240): many blocks
GT_SHAPES = [(3, 3), (8, 16), (37, 53), (64, 128), (135, 240)]
CANNY_SHAPES = [(3, 3), (5, 7), (37, 53), (64, 128), (135, 240)]
MASK_SHAPES = [(1, 1), (7, 9), (37, 53), (135, 240)]


def _seg_chw(shape, seed=0):
    return np.ascontiguousarray(seg_scene(*shape, seed=seed).transpose(2, 0, 1).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ cityscapes_gt
@pytest.mark.parametrize("with_seg", [True, False])
@pytest.mark.parametrize("shape", GT_SHAPES)
def test_cityscapes_gt_equals_the_numpy_decode(route, shape, with_seg):
    seg = seg_scene(*shape, seed=2)
    raw = disp_scene(seg, seed=2)
    raw[0, 0] = 0
    factor = cs_factor(1)
    want_d, want_b, want_s = decode_spec_cs(raw, seg if with_seg else None, factor)
    depth, boundary, seg_f = route.cityscapes_gt(torch.from_numpy(raw).to(DEV), torch.from_numpy(seg).to(DEV) if with_seg else None, factor)
    assert depth.dtype == torch.float32 and boundary.dtype == torch.uint8 and tuple(depth.shape) == tuple(boundary.shape) == shape
    assert bit_equal(depth.cpu().numpy(), want_d), (shape, with_seg)
    assert np.array_equal(boundary.cpu().numpy(), want_b), (shape, with_seg)
    assert (want_d == -1).any() and (want_d == 0).any()  # band pixels and zeros (invalid samples; with a map also the sky)
    if with_seg:
        assert seg_f.dtype == torch.float32 and tuple(seg_f.shape) == (3,) + shape and torch.equal(seg_f.cpu(), torch.from_numpy(want_s))
        if min(shape) > 8:
            sky = (seg[:, :, 0] == 70) & (seg[:, :, 1] == 130)
            assert sky.any() and (want_d[sky] == 0).all()
    else:
        assert seg_f is None
    if min(shape) > 8:
        assert want_b.sum() > 10 and (want_d > 0).any()
    again = route.cityscapes_gt(torch.from_numpy(raw).to(DEV), torch.from_numpy(seg).to(DEV) if with_seg else None, factor)
    assert torch.equal(again[0], depth) and torch.equal(again[1], boundary)


def test_sky_pixels_with_a_disparity_are_cleared(route):
    """a class mask over valid samples: 0 replaces the decoded depth, and the boundary map sees the 0"""
    seg = seg_scene(37, 53)
    raw = np.full((37, 53), 2561, np.uint16)
    want_d, want_b, _ = decode_spec_cs(raw, seg, 100.0)
    depth, boundary, _ = route.cityscapes_gt(torch.from_numpy(raw).to(DEV), torch.from_numpy(seg).to(DEV), 100.0)
    assert bit_equal(depth.cpu().numpy(), want_d) and np.array_equal(boundary.cpu().numpy(), want_b)
    assert set(np.unique(want_d)) == {-1.0, 0.0, 10.0} and want_b.sum() > 20
    plain = route.cityscapes_gt(torch.from_numpy(raw).to(DEV), None, 100.0)
    assert not (plain[0] == 0).any() and plain[1].sum() < boundary.sum()


def test_cityscapes_gt_routes_agree_and_reject_wrong_inputs(monkeypatch):
    from patchrefinerv2_amd import ops
    seg = seg_scene(135, 240, seed=1)
    raw = disp_scene(seg, seed=1)
    out = []
    for r in ("ctypes", "torch"):
        monkeypatch.setattr(ops, "DISPATCH", r)
        out.append(ops.cityscapes_gt(torch.from_numpy(raw).to(DEV), torch.from_numpy(seg).to(DEV), cs_factor(0)))
        out.append(ops.seg_canny(torch.from_numpy(_seg_chw((135, 240), 1)).to(DEV)))
        with pytest.raises(ValueError, match="uint16"):
            ops.cityscapes_gt(torch.zeros(4, 4, device=DEV), None, 1.0)
        with pytest.raises(ValueError, match="shape"):
            ops.cityscapes_gt(torch.zeros(4, 4, dtype=torch.uint16, device=DEV), torch.zeros(4, 5, 3, dtype=torch.uint8, device=DEV), 1.0)
    for a, b in zip(out[0], out[2]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)  # bits
    assert torch.equal(out[1], out[3])


# ------------------------------------------------------------------------------------------------------------------ seg_canny
@pytest.mark.parametrize("shape", CANNY_SHAPES)
def test_seg_canny_equals_the_spec_exactly(route, shape):
    seg = _seg_chw(shape, seed=shape[0])
    want = seg_canny_spec(seg)
    got = route.seg_canny(torch.from_numpy(seg).to(DEV))
    assert got.dtype == torch.bool and tuple(got.shape) == shape and got.is_cuda
    diff = int((got.cpu().numpy() != want).sum())
    print(f"{shape}: {int(want.sum())} edge pixels, {diff} differ")
    assert diff == 0, (shape, diff)
    assert torch.equal(route.seg_canny(torch.from_numpy(seg).to(DEV)), got)  # the same mask on every call
    if shape[0] >= 37:
        assert 0 < want.mean() < 1


def test_seg_canny_on_noise_and_wrong_inputs(route):
    """random colours: every pixel has a gradient of its own direction, all four axes and long weak chains are in play"""
    rs = np.random.RandomState(5)
    seg = rs.randint(0, 256, (3, 37, 53)).astype(np.float32)
    seg[:, 10:30, 20:40] *= np.float32(0.01)  # a quiet patch: magnitudes around the two thresholds
    want = seg_canny_spec(seg)
    got = route.seg_canny(torch.from_numpy(seg).to(DEV)).cpu().numpy()
    assert np.array_equal(got, want) and 0 < want.mean() < 1
    for shape in ((2, 9), (9, 2)):
        with pytest.raises(ValueError, match="3 x 3"):
            route.seg_canny(torch.zeros((3,) + shape, device=DEV))
    with pytest.raises(ValueError, match="GPU"):
        route.seg_canny(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="shape"):
        route.seg_canny(torch.zeros(1, 8, 8, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ cityscapes_masks
@pytest.mark.parametrize("shape", MASK_SHAPES)
def test_cityscapes_masks_equal_the_spec(route, shape):
    rs = np.random.RandomState(shape[0] * 31 + shape[1])
    for dens in (0.03, 0.3):
        s, g, r = rs.rand(*shape) < dens, rs.rand(*shape) < 0.02, rs.rand(*shape) < 0.3
        s.flat[0] = g.flat[-1] = True
        want_e, want_f = masks_spec(s, g, r)
        edge, flatten = route.cityscapes_masks(torch.from_numpy(s).to(DEV), torch.from_numpy(g).to(DEV), torch.from_numpy(r.astype(np.uint8)).to(DEV))
        assert edge.dtype == flatten.dtype == torch.uint8 and tuple(edge.shape) == tuple(flatten.shape) == shape
        assert np.array_equal(edge.cpu().numpy(), want_e.astype(np.uint8)) and np.array_equal(flatten.cpu().numpy(), want_f.astype(np.uint8)), (shape, dens)
        assert not (edge & flatten).any()
    with pytest.raises(ValueError, match="match"):
        route.cityscapes_masks(torch.zeros(4, 4, dtype=torch.bool, device=DEV), torch.zeros(4, 5, dtype=torch.bool, device=DEV),
                               torch.zeros(4, 4, dtype=torch.bool, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ dataset and CLI
def _model_lines():
    return (f"model = dict(config=dict(patch_process_shape={list(PPS)}, image_raw_shape={list(CS_SHAPE)}, patch_split_num={list(SPLIT)},\n"
            "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")


@pytest.fixture(scope="module")
def cs_run(tmp_path_factory):
    """a two-frame synthetic Cityscapes tree, the model (synthetic weights) and the dataset the CLI builds for its config, and one
    Tester.run; ``scored`` records what get_metrics was handed"""
    from patchrefinerv2_amd import models, weights as W  # noqa: F401
    from patchrefinerv2_amd.registry import Config, build_model
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    tmp = tmp_path_factory.mktemp("cityscapes")
    root = str(tmp / "data")
    split, items = write_cityscapes_tree(root, CS_FRAMES, CS_SHAPE, seed=CS_SEED)
    cfg_path = tmp / "cfg.py"
    cfg_path.write_text(cityscapes_config_text(root, split, extra=_model_lines()))
    cfg = Config.fromfile(str(cfg_path))
    mcfg = cfg.model.to_dict()
    mcfg["config"].update(prec="bf16x3", max_batch=41, n_streams=3)  # tools/test.py's defaults
    model = build_model(mcfg)
    model.load_state_dict(W.synth_state_dict(model.spec(), seed=0), strict=True)
    ds = cli_dataset(cfg_path, image_raw_shape=list(CS_SHAPE))  # as tools/test.py --test-type cityscapes builds it
    fetched = [ds[i] for i in (0, 1, 0)]  # in order (the read one ahead is used) and back (it is dropped)
    scored = []
    own = ds.get_metrics

    def recording(depth_gt, result, disp_gt_edges=None, **kw):
        scored.append((depth_gt.cpu(), result.cpu(), disp_gt_edges.cpu(), kw["image_hr"].cpu(), kw["seg_image"].cpu()))
        return own(depth_gt, result, disp_gt_edges=disp_gt_edges, **kw)
    ds.get_metrics = recording
    t = Tester(None, RunnerInfo(), ds, model)
    one = t.run(cai_mode="m1", image_raw_shape=CS_SHAPE, patch_split_num=SPLIT, seed=621, frame_batch=1)
    ds.close()
    return dict(tmp=tmp, root=root, split=split, cfg=str(cfg_path), ds=ds, items=items, fetched=fetched, one=one, scored=scored,
                last_eval=dict(t.last_eval))


def test_dataset_items_equal_the_spec(cs_run):
    ds, items = cs_run["ds"], cs_run["items"]
    assert len(ds) == CS_FRAMES and [i["img_path"] for i in ds.data_infos] == [it["img"] for it in items]
    for idx, item in zip((0, 1, 0), cs_run["fetched"]):
        it = items[idx]
        assert tuple(item) == ("image_hr", "depth_gt", "boundary", "img_file_basename", "seg_image")  # no image_lr
        assert item["img_file_basename"] == os.path.splitext(it["rel"])[0].replace("/", "_")
        want_img = np.ascontiguousarray((it["pixels"].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1))
        assert item["image_hr"].is_cuda and torch.equal(item["image_hr"].cpu(), torch.from_numpy(want_img)), idx
        want_d, want_b, want_s = decode_spec_cs(it["raw"], it["seg_u8"], it["factor"])
        assert tuple(item["depth_gt"].shape) == (1, 1) + CS_SHAPE and item["boundary"].dtype == torch.uint8
        assert bit_equal(item["depth_gt"][0, 0].cpu().numpy(), want_d) and np.array_equal(item["boundary"].cpu().numpy(), want_b)
        assert item["seg_image"].dtype == torch.float32 and torch.equal(item["seg_image"].cpu(), torch.from_numpy(want_s))
        assert want_b.sum() > 50 and (want_d == 0).any() and (want_d == -1).any() and (want_d > 0).any()
    assert cs_run["items"][0]["factor"] != cs_run["items"][1]["factor"]  # every frame decodes with its own camera


def test_dataset_without_a_segmentation_map_and_malformed_files(cs_run, tmp_path):
    from PIL import Image
    from patchrefinerv2_amd import tester
    tc = dict(degree=1.0, network_process_size=[384, 512])
    ds = tester.CityScapesDataset("infer", cs_run["split"], tc, 1e-3, 250, data_root=cs_run["root"])
    try:
        item = ds[1]
    finally:
        ds.close()
    it = cs_run["items"][1]
    assert tuple(item) == ("image_hr", "depth_gt", "boundary", "img_file_basename")
    want_d, want_b, _ = decode_spec_cs(it["raw"], None, it["factor"])
    assert bit_equal(item["depth_gt"][0, 0].cpu().numpy(), want_d) and np.array_equal(item["boundary"].cpu().numpy(), want_b)
    root = str(tmp_path / "bad")
    split, items = write_cityscapes_tree(root, 1, (8, 16))
    it = items[0]

    def fails(path):
        bad = tester.CityScapesDataset("infer", split, tc, 1e-3, 250, data_root=root, with_seg_map=True)
        try:
            with pytest.raises(ValueError, match=re.escape(path)):
                bad[0]
        finally:
            bad.close()
    Image.fromarray(it["seg_u8"][:, :-1]).save(it["seg"])
    fails(it["seg"])
    Image.fromarray(it["seg_u8"]).save(it["seg"])
    Image.fromarray(it["pixels"][:-1]).save(it["img"])
    fails(it["img"])
    Image.fromarray(it["pixels"]).save(it["img"])
    with open(it["camera"], "w") as f:
        f.write('{"extrinsic": {"pitch": 0.0}, "intrinsic": {"fx": 2262.52}}')
    fails(it["camera"])
    Image.fromarray((it["raw"] >> 8).astype(np.uint8)).save(it["disp"])
    fails(it["disp"])


def test_get_metrics_equals_the_host_metrics_on_the_spec_masks(cs_run):
    """cityscapes_dataset.py:360-403 on the host with the specification's masks, against Tester.run.  The prediction's own edge map is
    the device's (ops.canny of its log depth, pinned by tests/test_edges_gpu.py): the host's log and resize may differ from the
    device's in the last ulp and move an edge pixel, which is no property of the code under test here -- the edge and flatten sets,
    the valid pixels and their composition are."""
    from patchrefinerv2_amd import metrics as M
    one = cs_run["one"]
    assert [r["name"] for r in one] == [i["img_file_basename"] for i in cs_run["ds"].data_infos] and len(cs_run["scored"]) == CS_FRAMES
    for idx, (r, (gt, result, edges, image, seg)) in enumerate(zip(one, cs_run["scored"])):
        it = cs_run["items"][idx]
        assert r["shape"] == (1, 1) + OUT == tuple(result.shape) and tuple(gt.shape) == (1, 1) + CS_SHAPE  # scoring resizes the map
        assert torch.equal(seg, torch.from_numpy(decode_spec_cs(it["raw"], it["seg_u8"], it["factor"])[2]))
        g = gt[0, 0].numpy()
        region = edge_region_spec(image, *CS_SHAPE, 0.05)
        edge_spec, flatten_spec = masks_spec(seg_canny_spec(seg), M.extract_edges(g, "log"), region)
        valid = (g > 1e-3) & (g < 250)
        assert (edge_spec & valid).sum() > 50 and (flatten_spec & valid).sum() > 1000 and 0 < region.mean() < 0.5
        kw = dict(disp_gt_edges=edges.numpy(), min_depth_eval=1e-3, max_depth_eval=250, garg_crop=False, eigen_crop=False, dataset="")
        with np.errstate(invalid="ignore"):
            ref = dict(M.compute_metrics(gt, result.clone(), additional_mask=torch.from_numpy(flatten_spec), **kw))
        pred = F.interpolate(result.to(DEV), CS_SHAPE, mode="bilinear", align_corners=False)
        # the resize of :320-322 itself against torch's CPU kernel: four products and three sums per value, each rounding (or its
        # contraction) within one ulp of the largest value -- 8 ulp of the map's maximum bounds it with room
        host_pred = F.interpolate(result, CS_SHAPE, mode="bilinear", align_corners=False)
        assert float((pred.cpu() - host_pred).abs().max()) <= 8 * 2.0 ** -23 * float(host_pred.abs().max())
        pred_edges = M.extract_edges_device(pred, "log").cpu().numpy()
        ref.update(M.compute_boundary_metrics(edge_spec, pred_edges, valid))
        assert tuple(r["metrics"]) == tuple(ref) == KEYS17
        for k in KEYS17:
            print(f"{r['name']} {k}: device {float(r['metrics'][k])!r} host {float(ref[k])!r}")
        _close(r["metrics"], ref, r["name"])
        assert r["metrics"]["see"] > 0 and 0 < r["metrics"]["abs_rel"] < 1000 and 0 <= r["metrics"]["acc"] <= 1
        unmasked = M.compute_metrics(gt, result.clone(), **kw)
        assert float(unmasked["abs_rel"]) != r["metrics"]["abs_rel"]  # the flatten set is in play
    assert one[0]["metrics"] != one[1]["metrics"]


def test_last_eval_is_the_nanmean(cs_run):
    one, ev = cs_run["one"], cs_run["last_eval"]
    assert tuple(ev) == KEYS17
    for k in KEYS17:
        assert ev[k] == float(np.nanmean([r["metrics"][k] for r in one])), k


def test_cli_test_type_cityscapes_prints_the_seventeen_keys(cs_run):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), cs_run["cfg"], "--synthetic-weights", "--cai-mode", "m1",
                        "--test-type", "cityscapes", "--image-raw-shape", str(CS_SHAPE[0]), str(CS_SHAPE[1]), "--patch-split-num", "2", "2"],
                       capture_output=True, text=True, timeout=600, cwd=str(cs_run["tmp"]))
    assert r.returncode == 0, r.stderr[-2000:]

    def parse(text):
        return {k: float(v) for k, v in (kv.split(" ") for kv in text.split(", "))}
    for res in cs_run["one"]:
        assert f"{res['name']}: depth {(1, 1) + OUT}" in r.stdout
        line = re.search(rf"{res['name']}: (a1 .*)", r.stdout)
        assert line, r.stdout[-2000:]
        printed = parse(line.group(1))
        assert tuple(printed) == KEYS17
        for k, v in printed.items():
            assert abs(v - res["metrics"][k]) <= 1e-6 * max(1.0, abs(res["metrics"][k])), (k, v, res["metrics"][k])
    summary = [ln for ln in r.stdout.splitlines() if ln.startswith("[rank 0] a1 ")]
    assert len(summary) == 1, r.stdout[-2000:]
    printed = parse(summary[0][len("[rank 0] "):])
    assert tuple(printed) == KEYS17
    for k, v in printed.items():
        assert abs(v - cs_run["last_eval"][k]) <= 1e-4 * max(1.0, abs(cs_run["last_eval"][k])), (k, v)
