"""GPU: KittiDataset and ScanNetDataset -- csrc/evalgt.hip's depth16_gt kernel against the specification of
tests/test_kitti_scannet_host.py (depth bit for bit, the boundary map pixel for pixel, both grid mappings), the two datasets' items
against the PIL + numpy host route on synthetic trees, their get_metrics against metrics.compute_metrics on the host, and one
tools/test.py run per new test type.  Both dispatch routes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_general_gt_host import bit_equal  # noqa: E402
from test_kitti_scannet_host import (KB, KEYS10, KEYS30, KITTI_FRAMES, KITTI_SHAPE, SCANNET_CLI_DEPTH, SCANNET_CLI_IMG, SCANNET_CLI_SEED,  # noqa: E402
                                     SCANNET_DEPTH, SCANNET_FRAMES, SCANNET_IMG, cli_dataset, kitti_config_text, kitti_dense, kitti_host_route,
                                     scannet_config_text, scannet_host_route, scannet_samples, write_kitti_tree, write_scannet_tree)
from test_u4k_eval_gpu import PPS, SPLIT, _close, route  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
torch.set_grad_enabled(False)

# (source, window shape, (top, left)).  9 x 14 / 5 x 7 at (4, 3): an odd margin and W no multiple of 4 (scalar loads and stores);
# 8 x 16 / 4 x 8 at left 4: 8-byte loads; at left 2: 4-byte loads; at left 1: scalar loads under vector stores; whole maps; one pixel,
# one row, one column; KITTI's own 375 x 1242 (margin 13) and the even-margin 360 x 1224: many blocks
WINDOWS = [((9, 14), (5, 7), (4, 3)), ((8, 16), (4, 8), (2, 4)), ((8, 16), (4, 8), (3, 2)), ((8, 16), (4, 8), (4, 1)), ((8, 16), (8, 16), (0, 0)),
           ((7, 9), (7, 9), (0, 0)), ((1, 1), (1, 1), (0, 0)), ((3, 20), (1, 13), (2, 5)), ((20, 3), (13, 1), (5, 2)), ((375, 1242), KB, (23, 13)),
           (KITTI_SHAPE, KB, (8, 4))]
# (source, output): an upscale by no integer; exact ties in both axes; the tie at column 40 of 640 -> 1296; a downscale; the identity
# (vector path and not); one pixel; the datasets' own sizes; ScanNet's 480 x 640 -> 968 x 1296: many blocks
NEAREST = [((5, 7), (13, 15)), ((4, 4), (6, 6)), ((2, 640), (3, 1296)), ((9, 12), (4, 5)), ((8, 16), (8, 16)), ((7, 9), (7, 9)), ((1, 1), (3, 3)),
           (SCANNET_DEPTH, SCANNET_IMG), (SCANNET_CLI_DEPTH, SCANNET_CLI_IMG), ((480, 640), (968, 1296))]


def _samples(shape, seed, spread):
    """uint16 samples whose neighbours differ by about the boundary threshold (``spread`` raw units), with 0 and 65535 among them"""
    rs = np.random.RandomState(seed)
    raw = (5000 + rs.randint(0, spread, shape)).astype(np.uint16)
    raw.flat[rs.randint(0, raw.size, max(1, raw.size // 50))] = 0
    raw.flat[rs.randint(0, raw.size, max(1, raw.size // 50))] = 65535
    return raw


def _check(ops, raw, out_hw, divisor, spec_kw, **kw):
    from patchrefinerv2_amd import metrics as M
    want_d, want_b = M.depth16_decode_spec(raw, divisor, **spec_kw)
    depth, boundary = ops.depth16_gt(torch.from_numpy(raw).to(DEV), out_hw, divisor, **kw)
    assert depth.dtype == torch.float32 and boundary.dtype == torch.uint8 and tuple(depth.shape) == tuple(boundary.shape) == tuple(want_d.shape)
    assert bit_equal(depth.cpu().numpy(), want_d), (raw.shape, out_hw, kw)
    diff = int((boundary.cpu().numpy() != want_b).sum())
    assert diff == 0, (raw.shape, out_hw, kw, diff)
    again = ops.depth16_gt(torch.from_numpy(raw).to(DEV), out_hw, divisor, **kw)
    assert torch.equal(again[0].view(torch.int32), depth.view(torch.int32)) and torch.equal(again[1], boundary)  # the same bits on every call
    return want_d, want_b


# ------------------------------------------------------------------------------------------------------------------ depth16_gt
@pytest.mark.parametrize("src,win,at", WINDOWS)
def test_window_mapping_equals_the_spec(route, src, win, at):
    raw = _samples(src, src[0] * 131 + at[1], 600)
    raw[at[0], at[1]], raw[at[0] + win[0] - 1, at[1] + win[1] - 1] = 0, 65535  # both extremes inside the window
    want_d, want_b = _check(route, raw, win, 256.0, dict(window=at + win), window=at)
    assert want_d.max() == np.float32(65535) / np.float32(256) or win == (1, 1)
    if win[0] * win[1] > 30:
        assert 0 < want_b.mean() < 1  # both classes of pixels
    if win == src:  # the whole map: no window, no shape
        got = route.depth16_gt(torch.from_numpy(raw).to(DEV), None, 256.0)
        assert bit_equal(got[0].cpu().numpy(), want_d) and np.array_equal(got[1].cpu().numpy(), want_b)


@pytest.mark.parametrize("src,out", NEAREST)
def test_nearest_mapping_equals_the_spec(route, src, out):
    raw = _samples(src, src[0] * 17 + out[1], 2500)
    raw.flat[0], raw.flat[-1] = 0, 65535
    want_d, want_b = _check(route, raw, out, 1000.0, dict(out_hw=out), nearest=True)
    if src == out:  # equal sizes: the identity
        assert bit_equal(want_d, raw.astype(np.float32) / np.float32(1000))
    if out[0] * out[1] > 30:
        assert 0 < want_b.mean() < 1
    if out[0] >= src[0] and out[1] >= src[1]:
        assert want_d.max() == np.float32(65535) / np.float32(1000)


def test_nearest_mapping_equals_pil_itself(route):
    """the kernel against PIL's own resize, with no restatement between them"""
    for src, out in (((2, 640), (3, 1296)), ((4, 4), (6, 6)), (SCANNET_DEPTH, SCANNET_IMG), ((480, 640), (968, 1296))):
        raw = _samples(src, 5, 2500)
        want_d, want_b = scannet_host_route(raw, out)
        depth, boundary = route.depth16_gt(torch.from_numpy(raw).to(DEV), out, 1000.0, nearest=True)
        assert bit_equal(depth.cpu().numpy(), want_d) and np.array_equal(boundary.cpu().numpy(), want_b), (src, out)
    raw = _samples((375, 1242), 6, 600)
    want_d, want_b = kitti_host_route(raw)
    depth, boundary = route.depth16_gt(torch.from_numpy(raw).to(DEV), KB, 256.0, window=(23, 13))
    assert bit_equal(depth.cpu().numpy(), want_d) and np.array_equal(boundary.cpu().numpy(), want_b)


def test_boundary_threshold_is_strict_on_the_device(route):
    """exactly 1.0 m apart is no boundary, one raw unit more is (both divisors), and ``th`` reaches the kernel"""
    raw = np.array([[1000, 1256, 1513, 1513, 0]], np.uint16)
    assert route.depth16_gt(torch.from_numpy(raw).to(DEV), None, 256.0)[1].cpu().tolist() == [[0, 1, 1, 1, 1]]
    raw = np.array([[2000], [3000], [4001], [4001]], np.uint16)
    assert route.depth16_gt(torch.from_numpy(raw).to(DEV), None, 1000.0)[1].cpu()[:, 0].tolist() == [0, 1, 1, 0]
    assert route.depth16_gt(torch.from_numpy(raw).to(DEV), None, 1000.0, th=0.5)[1].cpu()[:, 0].tolist() == [1, 1, 1, 0]
    raw = np.array([[1000, 3000]], np.uint16)  # the output's neighbours, not the source's
    assert route.depth16_gt(torch.from_numpy(raw).to(DEV), (1, 6), 1000.0, nearest=True)[1].cpu().tolist() == [[0, 0, 1, 1, 0, 0]]
    raw = np.array([[9000, 1000, 1000, 9000]], np.uint16)  # a step at the window's edge is outside it
    assert route.depth16_gt(torch.from_numpy(raw).to(DEV), (1, 2), 256.0, window=(0, 1))[1].cpu().tolist() == [[0, 0]]


def test_routes_agree_and_reject_wrong_inputs(monkeypatch):
    from patchrefinerv2_amd import ops
    raw = torch.from_numpy(_samples((37, 53), 3, 600)).to(DEV)
    out = []
    for r in ("ctypes", "torch"):
        monkeypatch.setattr(ops, "DISPATCH", r)
        out.append(ops.depth16_gt(raw, (20, 31), 256.0, window=(5, 7)) + ops.depth16_gt(raw, (50, 41), 1000.0, nearest=True))
        with pytest.raises(ValueError, match="uint16"):
            ops.depth16_gt(torch.zeros(37, 53, device=DEV), (4, 4), 256.0)
        with pytest.raises(ValueError, match="GPU"):
            ops.depth16_gt(raw.cpu(), (4, 4), 256.0)
        with pytest.raises(ValueError, match=r"\[H, W\]"):
            ops.depth16_gt(raw[None], (4, 4), 256.0)
        with pytest.raises(ValueError, match="outside"):
            ops.depth16_gt(raw, (20, 31), 256.0, window=(18, 7))
        with pytest.raises(ValueError, match="outside"):
            ops.depth16_gt(raw, (38, 53), 256.0)
        with pytest.raises(ValueError, match="not both"):
            ops.depth16_gt(raw, (20, 31), 256.0, window=(0, 0), nearest=True)
        with pytest.raises(ValueError, match="not positive"):
            ops.depth16_gt(raw, (20, 31), 0.0)
        with pytest.raises(ValueError, match="bad shape"):
            ops.depth16_gt(raw, (0, 31), 256.0, nearest=True)
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)  # bits


# ------------------------------------------------------------------------------------------------------------------ the datasets' items
def _image_chw(pixels):
    return torch.from_numpy(np.ascontiguousarray((pixels.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)))


@pytest.fixture(scope="module")
def kitti_tree(tmp_path_factory):
    """a two-frame synthetic KITTI tree (frame 1: nothing valid inside the Garg crop), its config and the dataset the CLI builds"""
    tmp = tmp_path_factory.mktemp("kitti")
    root = str(tmp / "data")
    split, items = write_kitti_tree(root)
    cfg = tmp / "cfg.py"
    cfg.write_text(kitti_config_text(root, split, extra=_model_lines(KB)))
    ds = cli_dataset(cfg, "kitti")
    fetched = [ds[i] for i in (0, 1, 0)]  # in order (the read one ahead is used) and back (it is dropped)
    ds.close()
    return dict(tmp=tmp, root=root, split=split, cfg=str(cfg), ds=ds, items=items, fetched=fetched)


@pytest.fixture(scope="module")
def scannet_tree(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("scannet")
    split, items = write_scannet_tree(str(tmp / "data"))
    cfg = tmp / "cfg.py"
    cfg.write_text(scannet_config_text(split))
    ds = cli_dataset(cfg, "scannet")
    fetched = [ds[i] for i in (1, 0, 1)]  # out of order from the start
    ds.close()
    return dict(tmp=tmp, split=split, cfg=str(cfg), ds=ds, items=items, fetched=fetched)


def _model_lines(raw_shape):
    return (f"model = dict(config=dict(patch_process_shape={list(PPS)}, image_raw_shape={list(raw_shape)}, patch_split_num={list(SPLIT)},\n"
            "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")


def test_kitti_items_equal_the_host_route(kitti_tree):
    ds, items = kitti_tree["ds"], kitti_tree["items"]
    assert len(ds) == KITTI_FRAMES and [i["img_path"] for i in ds.data_infos] == [it["img"] for it in items]
    top, left = KITTI_SHAPE[0] - KB[0], (KITTI_SHAPE[1] - KB[1]) // 2
    for idx, item in zip((0, 1, 0), kitti_tree["fetched"]):
        it = items[idx]
        assert tuple(item) == ("image_hr", "depth_gt", "boundary", "img_file_basename")  # no image_lr
        assert item["img_file_basename"] == os.path.splitext(it["rel"])[0].replace("/", "_")
        want_img = _image_chw(it["pixels"][top:top + KB[0], left:left + KB[1]])
        assert item["image_hr"].is_cuda and tuple(item["image_hr"].shape) == (3,) + KB and torch.equal(item["image_hr"].cpu(), want_img), idx
        want_d, want_b = kitti_host_route(it["raw"])
        assert tuple(item["depth_gt"].shape) == (1, 1) + KB and item["depth_gt"].is_cuda and item["boundary"].dtype == torch.uint8
        assert bit_equal(item["depth_gt"][0, 0].cpu().numpy(), want_d) and np.array_equal(item["boundary"].cpu().numpy(), want_b), idx
        assert want_b.sum() > 50 and (want_d == 0).mean() > 0.5 and (want_d > 0).any()


def test_kitti_without_the_crop_and_malformed_files(kitti_tree, tmp_path):
    from PIL import Image
    from patchrefinerv2_amd import tester
    tc = dict(degree=1.0, network_process_size=[384, 512])
    ds = tester.KittiDataset("infer", kitti_tree["root"], kitti_tree["split"], tc, 1e-3, 80, do_kb_crop=False)
    try:
        item = ds[1]
    finally:
        ds.close()
    it = kitti_tree["items"][1]
    want_d, want_b = kitti_host_route(it["raw"], do_kb_crop=False)
    assert tuple(item["depth_gt"].shape) == (1, 1) + KITTI_SHAPE and torch.equal(item["image_hr"].cpu(), _image_chw(it["pixels"]))
    assert bit_equal(item["depth_gt"][0, 0].cpu().numpy(), want_d) and np.array_equal(item["boundary"].cpu().numpy(), want_b)
    root = str(tmp_path / "bad")
    split, items = write_kitti_tree(root, n=1)
    it = items[0]

    def fails(path):
        bad = tester.KittiDataset("infer", root, split, tc, 1e-3, 80)
        try:
            with pytest.raises(ValueError, match=re.escape(path)):
                bad[0]
        finally:
            bad.close()
    Image.fromarray(it["pixels"][:, :-1]).save(it["img"])
    fails(it["img"])
    Image.fromarray(it["pixels"]).save(it["img"])
    Image.fromarray((it["raw"] >> 8).astype(np.uint8)).save(it["depth"])
    fails(it["depth"])


def test_scannet_items_equal_the_host_route(scannet_tree):
    ds, items = scannet_tree["ds"], scannet_tree["items"]
    assert len(ds) == SCANNET_FRAMES and [i["img_path"] for i in ds.data_infos] == [it["img"] for it in items]
    for idx, item in zip((1, 0, 1), scannet_tree["fetched"]):
        it = items[idx]
        assert tuple(item) == ("image_hr", "depth_gt", "boundary", "img_file_basename")
        assert item["img_file_basename"] == f"1ada7a0617_{120 * idx:06d}"
        assert item["image_hr"].is_cuda and torch.equal(item["image_hr"].cpu(), _image_chw(it["pixels"])), idx
        want_d, want_b = scannet_host_route(it["raw"], SCANNET_IMG)  # the outputs have the image's size
        assert tuple(item["depth_gt"].shape) == (1, 1) + SCANNET_IMG and item["boundary"].dtype == torch.uint8
        assert bit_equal(item["depth_gt"][0, 0].cpu().numpy(), want_d) and np.array_equal(item["boundary"].cpu().numpy(), want_b), idx
        assert want_b.sum() > 20 and (want_d == 0).any()
    assert not np.array_equal(items[0]["raw"], items[1]["raw"])


# ------------------------------------------------------------------------------------------------------------------ get_metrics
def _kitti_predictions(seed):
    """a prediction of the ground truth's size and one of another size, on the device: the dense scene 10 % off, with a NaN, an inf and a
    negative value inside the Garg crop"""
    same = (kitti_dense(*KB, seed) * 1.1).astype(np.float32)
    same[200, 300], same[210, 310], same[220, 320] = np.nan, np.inf, -1.0
    low = (kitti_dense(KB[0] // 2, KB[1] // 2, seed) * 0.9).astype(np.float32)
    return [torch.from_numpy(p)[None, None].to(DEV) for p in (same, low)]


def test_kitti_get_metrics_equals_the_host_inside_the_garg_crop(kitti_tree):
    from patchrefinerv2_amd import metrics as M
    ds = kitti_tree["ds"]
    item = kitti_tree["fetched"][0]
    gt, edges = item["depth_gt"].cpu(), item["boundary"].cpu()
    kw = dict(disp_gt_edges=edges, min_depth_eval=1e-3, max_depth_eval=80, garg_crop=True, eigen_crop=False, dataset="kitti")
    rows = []
    for pred in _kitti_predictions(0):
        got = ds.get_metrics(item["depth_gt"], pred, disp_gt_edges=item["boundary"], image_hr=item["image_hr"])
        ref = M.compute_metrics(gt, pred.cpu().clone(), **kw)
        assert tuple(got) == tuple(ref) == KEYS10
        for k in KEYS10:
            print(f"{tuple(pred.shape[-2:])} {k}: device {float(got[k])!r} host {float(ref[k])!r}")
        _close(got, ref, str(tuple(pred.shape)))
        assert got["see"] > 0 and 0 < got["abs_rel"] < 1 and 0 < got["a1"] <= 1
        uncropped = M.compute_metrics(gt, pred.cpu().clone(), **dict(kw, garg_crop=False))
        assert float(uncropped["rmse"]) != got["rmse"]  # the crop is in play
        rows.append(got)
    assert rows[0] != rows[1]


def test_kitti_empty_garg_crop_gives_nan_and_a_finite_evaluate(kitti_tree):
    from patchrefinerv2_amd import metrics as M
    ds = kitti_tree["ds"]
    full, empty = kitti_tree["fetched"][0], kitti_tree["fetched"][1]
    pred = _kitti_predictions(1)[1]
    got = ds.get_metrics(empty["depth_gt"], pred, disp_gt_edges=empty["boundary"])
    assert tuple(got) == KEYS10 and all(np.isnan(got[k]) for k in KEYS10[:-1]) and got["see"] == 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = M.compute_metrics(empty["depth_gt"].cpu(), pred.cpu().clone(), disp_gt_edges=empty["boundary"].cpu(), min_depth_eval=1e-3,
                                    max_depth_eval=80, garg_crop=True, eigen_crop=False, dataset="kitti")
    _close(got, ref, "empty crop")  # (NaN where the host has NaN)
    assert bool(((empty["depth_gt"] > 1e-3) & (empty["depth_gt"] < 80)).any())  # the frame itself has returns, above the crop
    other = ds.get_metrics(full["depth_gt"], pred, disp_gt_edges=full["boundary"])
    ev = ds.evaluate([other, got])
    assert tuple(ev) == KEYS10 and all(np.isfinite(v) for v in ev.values())
    assert all(ev[k] == other[k] for k in KEYS10[:-1]) and ev["see"] == other["see"] / 2


def test_ssi_keys_follow(kitti_tree, scannet_tree):
    from patchrefinerv2_amd import metrics as M
    for tree, kind, keys, crop in ((kitti_tree, "kitti", KEYS10, dict(garg_crop=True, dataset="kitti")), (scannet_tree, "scannet", KEYS30, dict(dataset=""))):
        ds = cli_dataset(tree["cfg"], kind, ssi_metrics=True)
        item = tree["fetched"][0]
        pred = (item["depth_gt"] * 1.3 + 0.2).contiguous()
        got = ds.get_metrics(item["depth_gt"], pred, disp_gt_edges=item["boundary"])
        assert tuple(got) == keys + M.SSI_KEYS
        want = M.compute_ssi_metrics_fused(item["depth_gt"], pred, min_depth_eval=1e-3, max_depth_eval=80, eigen_crop=False, fuse_resize=True, **crop)
        assert {k: got[k] for k in M.SSI_KEYS} == want and abs(got["ssi_scale"] - 1 / 1.3) < 1e-4
        plain = tree["ds"].get_metrics(item["depth_gt"], pred, disp_gt_edges=item["boundary"])
        assert tuple(plain) == keys and all(got[k] == plain[k] or (np.isnan(got[k]) and np.isnan(plain[k])) for k in keys)


def test_scannet_region_and_thirty_keys_equal_the_host(scannet_tree):
    """scannet_dataset.py:221-243 on the host -- metrics.edge_split_masks and three compute_metrics calls -- against one get_metrics
    (tests/test_kitti_scannet_host.py asserts that no pixel of these scenes is near a Canny threshold)"""
    from patchrefinerv2_amd import metrics as M
    ds = scannet_tree["ds"]
    for idx, item in zip((1, 0), scannet_tree["fetched"][:2]):
        gt = item["depth_gt"].cpu()
        g = gt[0, 0].numpy()
        region = M.edge_split_masks(g)
        got_region = M.edge_split_masks_device(item["depth_gt"][0, 0], 7).cpu().numpy().astype(bool)
        diff = int((got_region != region).sum())
        print(f"frame {idx}: region {int(region.sum())} pixels, {diff} differ")
        assert got_region.shape == SCANNET_IMG and diff == 0
        valid = (g > 1e-3) & (g < 80)
        assert (region & valid).sum() > 50 and (~region & valid).sum() > 50
        low = torch.from_numpy(scannet_samples(15, 20, seed=idx).astype(np.float32) / np.float32(1000) * np.float32(0.93))[None, None]
        # the prediction of the ground truth's size is off by a factor that varies across the frame: under a constant factor the log
        # error is nearly constant, silog = sqrt(E[err^2] - E[err]^2) cancels 220-fold and the HOST's float32 sums miss the float64
        # value (which the device gives) by 2.3e-5, more than _close allows
        ramp = torch.linspace(0.9, 1.2, SCANNET_IMG[1], device=DEV)
        for pred in ((item["depth_gt"] * ramp + 0.05).contiguous(), low.to(DEV)):
            got = ds.get_metrics(item["depth_gt"], pred, disp_gt_edges=item["boundary"])  # (it needs no image_hr)
            kw = dict(disp_gt_edges=item["boundary"].cpu(), min_depth_eval=1e-3, max_depth_eval=80, garg_crop=False, eigen_crop=False, dataset="")
            ref = {}
            for pre, mask in (("edge_", torch.from_numpy(region)), ("noedge_", torch.from_numpy(~region)), ("", None)):
                ref.update({pre + k: v for k, v in M.compute_metrics(gt, pred.cpu().clone(), additional_mask=mask, **kw).items()})
            assert tuple(got) == tuple(ref) == KEYS30
            for k in KEYS30:
                print(f"frame {idx} {tuple(pred.shape[-2:])} {k}: device {float(got[k])!r} host {float(ref[k])!r}")
            _close(got, ref, f"frame {idx} {tuple(pred.shape)}")
            assert got["edge_abs_rel"] != got["noedge_abs_rel"] and got["see"] > 0
    ev = ds.evaluate([got, got])
    assert tuple(ev) == KEYS30 and ev == {k: float(v) for k, v in got.items()}


# ------------------------------------------------------------------------------------------------------------------ the command line
def _parse(text):
    return {k: float(v) for k, v in (kv.split(" ") for kv in text.split(", "))}


def _cli(cfg, kind, raw_shape, cwd, names, keys, extra=()):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), cfg, "--synthetic-weights", "--cai-mode", "m1", "--test-type", kind,
                        "--image-raw-shape", str(raw_shape[0]), str(raw_shape[1]), "--patch-split-num", str(SPLIT[0]), str(SPLIT[1])] + list(extra),
                       capture_output=True, text=True, timeout=600, cwd=cwd)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = []
    for name in names:
        line = re.search(rf"{name}: ({keys[0]} .*)", r.stdout)
        assert line, r.stdout[-2000:]
        rows.append(_parse(line.group(1)))
        assert tuple(rows[-1]) == keys
    summary = [ln for ln in r.stdout.splitlines() if ln.startswith(f"[rank 0] {keys[0]} ")]
    assert len(summary) == 1, r.stdout[-2000:]
    ev = _parse(summary[0][len("[rank 0] "):])
    assert tuple(ev) == keys
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        for k in keys:  # the dataset's evaluate: the nanmean of the printed rows (six and four decimals)
            want = float(np.nanmean([row[k] for row in rows]))
            assert abs(ev[k] - want) <= 1e-4 * max(1.0, abs(want)) + 1e-6 or (np.isnan(ev[k]) and np.isnan(want)), (k, ev[k], want)
    return rows, ev


def test_cli_test_type_kitti_prints_the_ten_keys(kitti_tree):
    names = [i["img_file_basename"] for i in kitti_tree["ds"].data_infos]
    rows, ev = _cli(kitti_tree["cfg"], "kitti", KB, str(kitti_tree["tmp"]), names, KEYS10)
    assert all(np.isfinite(rows[0][k]) for k in KEYS10) and rows[0]["see"] > 0
    assert all(np.isnan(rows[1][k]) for k in KEYS10[:-1])  # frame 1: an empty Garg crop
    assert all(np.isfinite(ev[k]) for k in KEYS10)         # ... which does not poison the mean


def test_cli_test_type_scannet_prints_the_thirty_keys(tmp_path):
    split, items = write_scannet_tree(str(tmp_path / "data"), img_shape=SCANNET_CLI_IMG, depth_shape=SCANNET_CLI_DEPTH, seed=SCANNET_CLI_SEED)
    cfg = tmp_path / "cfg.py"
    cfg.write_text(scannet_config_text(split, extra=_model_lines(SCANNET_CLI_IMG)))
    names = [f"1ada7a0617_{120 * i:06d}" for i in range(SCANNET_FRAMES)]
    out = tmp_path / "out"  # --save sees ordinary items: the files carry the reference's basenames
    rows, ev = _cli(str(cfg), "scannet", SCANNET_CLI_IMG, str(tmp_path), names, KEYS30, extra=("--save", "--work-dir", str(out)))
    assert all(os.path.getsize(out / f"{n}{suffix}") > 0 for n in names for suffix in (".png", "_uint16.png"))
    assert all(np.isfinite(rows[i][k]) for i in range(SCANNET_FRAMES) for k in KEYS30) and rows[0] != rows[1]
