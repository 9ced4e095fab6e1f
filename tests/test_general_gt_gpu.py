"""GPU: the general dataset's ground truth -- csrc/evalgt.hip's gt_decode_kernel against the numpy spec of tests/test_general_gt_host.py
(which is pinned to the reference's outputs), the low-resolution scoring kernel against interpolate-then-score, and
tester.ImageDataset(gt_format=...) through Tester.run and tools/test.py --test-type general.  Both dispatch routes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from test_general_gt_host import CITYSCAPES_FACTOR, bit_equal, decode_spec, write_general_tree  # noqa: E402
from test_u4k_eval_gpu import MN, MX, OUT, PPS, RAW, SPLIT, _close, check_sums, ref_sums, route  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
torch.set_grad_enabled(False)
SHAPES = [(1, 1), (2, 3), (5, 1), (37, 53), (270, 480)]  # one pixel; tiny; one column; a scalar tail; float4 rows over many blocks
NATIVE_LITTLE = sys.byteorder == "little"


# ------------------------------------------------------------------------------------------------------------------ gt_decode
def _float_map(shape, seed):
    """smooth values with steps above th on every frame border and in every corner, a step of exactly th = 1 and one an ulp above,
    and 0, NaN, +inf, -inf samples; no two rows alike (the flip of a PFM payload shows)"""
    h, w = shape
    rs = np.random.RandomState(seed)
    d = (5.0 + 0.3 * rs.rand(h, w) + 0.01 * np.arange(h)[:, None]).astype(np.float32)
    d[0, ::2] += 3.0
    d[-1, 1::2] += 3.0
    d[::2, 0] += 3.0
    d[1::2, -1] += 3.0
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        d[y, x] += 7.0
    if h * w > 6 and w > 8:
        d[h // 2, w // 2] = 0.0
        d[h // 3, w // 3] = np.nan
        d[h // 4, w // 2], d[h // 4 + 1, w // 4] = np.inf, -np.inf
        r = (2 * h) // 3
        d[r - 1:r + 2, 2:8] = 5.25                                   # a flat patch: the only steps in it are the two below
        d[r, 3] = 6.25                                               # exactly th: no edge
        d[r, 6] = np.nextafter(np.float32(6.25), np.float32(np.inf))  # one ulp above th: an edge
    return d


def _u16_map(shape, seed):
    """Cityscapes samples: two planes, noise, the samples 0 / 1 / 65535, steps on the borders and corners, and a flat patch with one
    sample next to its neighbours' value (the depth step that the test uses as th)"""
    h, w = shape
    rs = np.random.RandomState(seed)
    v = (3000 + 4000 * (np.arange(w)[None, :] > w * 0.45) + rs.randint(0, 60, (h, w)) + 3 * np.arange(h)[:, None]).astype(np.uint16)
    v[0, ::2] += 900
    v[-1, 1::2] += 900
    v[::2, 0] += 900
    v[1::2, -1] += 900
    v[0, 0], v[-1, -1] = 65535, 1
    if h * w > 6 and w > 8:
        v[h // 2, w // 2], v[h // 3, w // 3], v[h // 4, w // 2] = 0, 1, 65535
        r = (2 * h) // 3
        v[r - 1:r + 2, 2:8] = 5000
        v[r, 4] = 5001
    return v


def _check_decode(ops, kind, src_dev, spec_src, ths, **kw):
    for th in ths:
        depth, boundary = ops.gt_decode(src_dev, kind, th=th, **kw)
        spec_kw = {k: v for k, v in kw.items() if k in ("factor", "doffs")}
        want_d, want_b = decode_spec(kind, spec_src, th=th, **spec_kw)
        assert depth.dtype == torch.float32 and boundary.dtype == torch.uint8 and tuple(depth.shape) == tuple(boundary.shape) == spec_src.shape
        assert bit_equal(depth.cpu().numpy(), want_d), (kind, spec_src.shape, th)
        assert np.array_equal(boundary.cpu().numpy(), want_b), (kind, spec_src.shape, th)
    return want_b


@pytest.mark.parametrize("shape", SHAPES)
def test_gt_decode_eth3d(route, shape):
    d = _float_map(shape, 3)
    edges = _check_decode(route, "eth3d", torch.from_numpy(d).to(DEV), d, (1.0, 0.25))
    if shape[1] > 8:
        r = (2 * shape[0]) // 3
        want = decode_spec("eth3d", d)[1]
        assert not want[r, 3] and not want[r, 4] and want[r, 5] and want[r, 6] and want[r, 7]  # th itself is no edge
        assert want[0, 0] and want[0, -1] and want[-1, 0] and want[-1, -1] and edges.sum() > 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("little", [True, False])
def test_gt_decode_middlebury_flip_and_byte_order(route, shape, little):
    d = _float_map(shape, 5) * np.float32(4.0)
    if shape[1] > 8:
        r = (2 * shape[0]) // 3
        d[r - 1:r + 2, 2:8], d[r, 3], d[r, 6] = 5.25, 6.25, np.nextafter(np.float32(6.25), np.float32(np.inf))
        d[1, 1] = np.float32(-131.111)  # disp + doffs == 0: the division by zero stays inf
    payload = np.flipud(d).astype("<f4" if little else ">f4").tobytes()  # a PFM payload: rows bottom to top, the file's byte order
    src = torch.from_numpy(np.frombuffer(payload, dtype=np.float32).reshape(shape).copy()).to(DEV)
    kw = dict(factor=193.001 * 3997.684, doffs=131.111, flip=True, byteswap=little != NATIVE_LITTLE)
    _check_decode(route, "mid", src, d, (1.0,), **kw)
    if shape[0] > 1:  # the flip matters: the unflipped decode is the spec of the flipped map
        depth, boundary = route.gt_decode(src, "mid", **dict(kw, flip=False))
        want_d, want_b = decode_spec("mid", np.flipud(d), factor=kw["factor"], doffs=kw["doffs"])
        assert bit_equal(depth.cpu().numpy(), want_d) and np.array_equal(boundary.cpu().numpy(), want_b)
        assert not bit_equal(want_d, decode_spec("mid", d, factor=kw["factor"], doffs=kw["doffs"])[0])
    if shape[1] > 8:
        depth = route.gt_decode(src, "mid", **kw)[0].cpu().numpy()
        assert depth[shape[0] // 4, shape[1] // 2] == 0 and np.isinf(depth[1, 1]) and np.isnan(depth[shape[0] // 3, shape[1] // 3])


@pytest.mark.parametrize("shape", SHAPES)
def test_gt_decode_cityscapes(route, shape):
    v = _u16_map(shape, 7)
    ths = [1.0]
    if shape[1] > 8:  # the depth step between the samples 5000 and 5001 as th, and the float below it
        dep = decode_spec("cityscapes", np.array([[5000, 5001]], np.uint16))[0][0]
        step = np.abs(dep[0] - dep[1])
        ths += [float(step), float(np.nextafter(step, np.float32(0)))]
    src = torch.from_numpy(v).to(DEV)
    _check_decode(route, "cityscapes", src, v, ths)
    if shape[1] > 8:
        r = (2 * shape[0]) // 3
        at, below = (decode_spec("cityscapes", v, th=t)[1] for t in ths[1:])
        assert not at[r, 3:6].any() and below[r, 3:6].all()  # a step of exactly th is no edge, one float more is
        depth = route.gt_decode(src, "cityscapes")[0].cpu().numpy()
        assert depth[shape[0] // 2, shape[1] // 2] == 0 and depth[shape[0] // 3, shape[1] // 3] == 0 and depth[-1, -1] == 0
        assert depth[0, 0] == np.float32(CITYSCAPES_FACTOR) / (np.float32(65534) / np.float32(256))
    # another factor and the other byte order of the samples
    _check_decode(route, "cityscapes", torch.from_numpy(v.byteswap()).to(DEV), v, (1.0,), factor=100.0, byteswap=True)


def test_gt_decode_rejects_wrong_inputs(route):
    f = torch.zeros(4, 4, device=DEV)
    with pytest.raises(ValueError):
        route.gt_decode(f, "cityscapes")
    with pytest.raises(ValueError):
        route.gt_decode(f.to(torch.uint16), "eth3d")
    with pytest.raises(ValueError):
        route.gt_decode(f[None], "eth3d")


# ------------------------------------------------------------------------------------------------------------------ depth_metrics_lowres
RATIOS = np.array([0.7, 0.9, 1.1, 1.4, 1.7, 2.2], np.float32)  # gt / prediction: each at least 8 % from 1.25^-k .. 1.25^k
LOWRES = [((19, 27), (37, 53)), ((1, 1), (5, 7)), ((80, 96), (37, 53)), ((135, 240), (270, 480))]


def _resize_cpu(lo, shape):
    return F.interpolate(torch.from_numpy(lo)[:, None], shape, mode="bilinear", align_corners=False)[:, 0].numpy()


def _lowres_case(lo_shape, shape, seed):
    """B = 2: a smooth low-resolution prediction with a NaN, and a ground truth built FROM its resized map times a ratio out of
    RATIOS (so every valid pixel's ratio is far from the thresholds), with invalid pixels; boundary, region and the garg crop"""
    from patchrefinerv2_amd import metrics as M
    (h, w), (H, W) = lo_shape, shape
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    lo = np.stack([1.0 + 1.5 * rs.rand() + 0.8 * np.sin(x / 5.0 + f) * np.cos(y / 4.0) + 0.2 * rs.rand(h, w) + 0.9 for f in range(2)]).astype(np.float32)
    up = _resize_cpu(lo, shape)
    gt = (up * RATIOS[rs.randint(0, len(RATIOS), (2, H, W))]).astype(np.float32)
    gf = gt.reshape(2, -1)
    n = max(1, H * W // 40)
    for f in range(2):
        idx = rs.permutation(H * W)
        gf[f, idx[:n]], gf[f, idx[n:2 * n]], gf[f, idx[2 * n:3 * n]] = 0.0, 30.0, np.inf
        if f == 1:  # (a NaN beside a boundary pixel makes the frame's soft-edge sum NaN, as np.minimum does: frame 0 keeps a number)
            gf[f, idx[3 * n:4 * n]] = np.nan
    if h * w > 6:
        lo[0, h // 2, w // 2] = np.nan  # (after gt was built: the resized NaNs clamp to min, ratio >= 7)
    with np.errstate(divide="ignore", invalid="ignore"):
        boundary = np.stack([M.get_boundaries(np.float32(40.0) / g, th=1.0, dilation=0) for g in gt]).astype(np.uint8)
    boundary[:, 0, :] = boundary[:, -1, :] = 1
    boundary[:, :, 0] = boundary[:, :, -1] = 1
    region = (rs.rand(2, H, W) < 0.4).astype(np.uint8)
    return gt, lo, boundary, region, M._eval_crop(H, W, True, False, "")


def _assert_far_from_thresholds(gt, lo):
    """the condition under which a one-ulp difference between two resizes cannot move a count: with torch's CPU resize, every valid
    pixel's ratio is >= 1 % from 1.25, 1.25^2, 1.25^3 and every finite gt >= 1 % from min / max"""
    up = _resize_cpu(lo, gt.shape[-2:])
    with np.errstate(invalid="ignore", divide="ignore"):
        up = np.clip(np.where(np.isnan(up), np.float32(MN), up), np.float32(MN), np.float32(MX)).astype(np.float64)
        g = gt.astype(np.float64)
        valid = (g > MN) & (g < MX)
        ratio = np.maximum(g / up, up / g)[valid]
        for t in (1.25, 1.25 ** 2, 1.25 ** 3):
            assert np.abs(ratio / t - 1).min() >= 0.01, t
        fin = g[np.isfinite(g) & (g > 0)]
        assert np.abs(fin / MN - 1).min() >= 0.01 and np.abs(fin / MX - 1).min() >= 0.01
    assert valid.sum() >= 0.5 * valid.size


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def test_lowres_on_equal_shapes_is_depth_metrics(route):
    for shape in ((37, 53), (270, 480)):
        gt, lo, boundary, region, crop = _lowres_case(shape, shape, 3)
        lo[1, 3, 5], lo[1, 4, 6], lo[0, 5, 7] = np.inf, -1.0, 50.0
        g, p, b, r = _dev(gt, lo, boundary, region)
        for args in ((g, p, b, r, MN, MX, crop), (g, p, b, None, MN, MX, None), (g, p, None, r, MN, MX, crop)):
            same = route.depth_metrics(*args)
            assert torch.equal(route.depth_metrics_lowres(*args).view(torch.int64), same.view(torch.int64))
            assert same[:, :, 0].min() > 0


@pytest.mark.parametrize("lo_shape,shape", LOWRES)
def test_lowres_against_interpolate_then_score(route, lo_shape, shape):
    from patchrefinerv2_amd import metrics as M
    gt, lo, boundary, region, crop = _lowres_case(lo_shape, shape, 11 + shape[0])
    _assert_far_from_thresholds(gt, lo)
    g, p, b, r = _dev(gt, lo, boundary, region)
    got = route.depth_metrics_lowres(g, p, b, r, MN, MX, crop)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 3, 12)
    assert torch.equal(route.depth_metrics_lowres(g, p, b, r, MN, MX, crop).view(torch.int64), got.view(torch.int64))  # the same bits on every call
    up = F.interpolate(p[:, None], shape, mode="bilinear", align_corners=False)[:, 0]
    two_step = route.depth_metrics(g, up, b, r, MN, MX, crop).cpu().numpy()
    up = up.cpu().numpy()
    for f in range(2):
        want, mag = ref_sums(gt[f], up[f], boundary[f], region[f], crop=crop)
        print(f"{lo_shape}->{shape} frame {f}: max |lowres - ref| / mag = {np.nanmax(np.abs(got[f].cpu().numpy() - want) / np.maximum(mag, 1e-300)):.3e}, "
              f"max |lowres - two-step| = {np.nanmax(np.abs(got[f].cpu().numpy() - two_step[f])):.3e}")
        check_sums(got[f].cpu().numpy(), want, mag, (lo_shape, shape, f))
        assert want[0, 0] > 0 and want[0, 10] > 0 and want[1, 0] > 0 and want[2, 0] > 0  # every set and the soft-edge term are in play
    # without a region / boundary / crop
    got1 = route.depth_metrics_lowres(g, p, None, None, MN, MX).cpu().numpy()
    for f in range(2):
        want, mag = ref_sums(gt[f], up[f])
        check_sums(got1[f], want, mag, (lo_shape, shape, f, "plain"))
    # the metric dicts: fused with the resize inside against the host's compute_metrics (torch's CPU resize)
    tg, tp = torch.from_numpy(gt)[:, None], torch.from_numpy(lo)[:, None]
    te, tr = torch.from_numpy(boundary.astype(np.float32)), torch.from_numpy(region.astype(bool))
    kw = dict(garg_crop=True, eigen_crop=False, dataset="", min_depth_eval=MN, max_depth_eval=MX)
    rows = M.compute_metrics_fused(tg, tp.to(DEV), disp_gt_edges=te, fuse_resize=True, **kw)
    rows_in = M.compute_metrics_fused(tg, tp.to(DEV), disp_gt_edges=te, additional_mask=tr, fuse_resize=True, **kw)
    default = M.compute_metrics_fused(tg, tp.to(DEV), disp_gt_edges=te, **kw)
    assert isinstance(rows, list) and len(rows) == 2
    for f in range(2):
        _close(rows[f], M.compute_metrics(tg[f:f + 1], tp[f:f + 1].clone(), disp_gt_edges=te[f], **kw), f"{shape} frame {f}")
        _close(rows_in[f], M.compute_metrics(tg[f:f + 1], tp[f:f + 1].clone(), disp_gt_edges=te[f], additional_mask=tr[f], **kw), f"{shape} in {f}")
        _close(rows[f], default[f], "fuse_resize against the default route")
    assert rows[0]["see"] > 0  # (frame 1 may hold a NaN gt pixel beside a boundary pixel: np.minimum propagates it)


def test_fuse_resize_with_equal_shapes_is_the_old_route():
    from patchrefinerv2_amd import metrics as M
    gt, lo, boundary, region, _ = _lowres_case((37, 53), (37, 53), 5)
    tg, tp, te = torch.from_numpy(gt)[:, None], torch.from_numpy(lo)[:, None].to(DEV), torch.from_numpy(boundary)
    kw = dict(garg_crop=False, eigen_crop=False, min_depth_eval=MN, max_depth_eval=MX, disp_gt_edges=te)
    assert repr(M.compute_metrics_fused(tg, tp, fuse_resize=True, **kw)) == repr(M.compute_metrics_fused(tg, tp, **kw))  # (repr: frame 1's see is NaN)


# ------------------------------------------------------------------------------------------------------------------ datasets
def _dataset(img_dir, gt_dir, **kw):
    from patchrefinerv2_amd import tester  # noqa: F401
    from patchrefinerv2_amd.registry import DATASETS
    return DATASETS.build(dict(type="ImageDataset", rgb_image_dir=img_dir, gt_dir=gt_dir, **kw))


@pytest.mark.parametrize("fmt", ["u4k", "eth3d", "mid", "cityscapes"])
def test_dataset_items_equal_the_spec(tmp_path, fmt):
    from patchrefinerv2_amd import datasets as T
    shape = (64, 96)
    img_dir, gt_dir, specs = write_general_tree(str(tmp_path), fmt, shape, n=3)
    ds = _dataset(img_dir, gt_dir, gt_format=fmt, gt_shape=shape, image_resolution=shape)
    try:
        for i in (0, 1, 2, 0, 2, 1):  # in order (the read one ahead is used) and out of it (it is dropped)
            item = ds[i]
            want_d, want_b = decode_spec(**specs[i])
            assert item["img_file_basename"] == f"frame_{i:03d}.npy" and set(item) == {"image_hr", "img_file_basename", "depth_gt", "boundary"}
            assert item["depth_gt"].is_cuda and tuple(item["depth_gt"].shape) == (1, 1) + shape and item["boundary"].dtype == torch.uint8
            assert bit_equal(item["depth_gt"][0, 0].cpu().numpy(), want_d), (fmt, i)
            assert np.array_equal(item["boundary"].cpu().numpy(), want_b) and want_b.sum() > 50, (fmt, i)
            ref = T.read_image_device(os.path.join(img_dir, f"frame_{i:03d}.npy"), shape)
            assert torch.equal(item["image_hr"], ref) and tuple(ref.shape) == (3,) + shape
        with pytest.raises(IndexError):
            ds[3]
    finally:
        ds.close()


def test_dataset_image_formats(tmp_path):
    from PIL import Image
    shape = (16, 24)
    rs = np.random.RandomState(1)
    px = rs.randint(0, 256, (375, 1242, 3)).astype(np.uint8)
    for fmt, name in (("cityscapes", "a.png"), ("kitti", "a.png"), ("u4k", "a.raw")):
        root = tmp_path / fmt
        _, gt_dir, specs = write_general_tree(str(root), "cityscapes", shape, n=1)
        img_dir = root / "rgb"
        os.makedirs(img_dir)
        if fmt == "u4k":
            px[:shape[0], :shape[1]].tofile(img_dir / name)
            want = px[:shape[0], :shape[1]].astype(np.float32)[:, :, ::-1].copy() / 255.0  # general_dataset.py:24-25
        else:
            Image.fromarray(px).save(img_dir / name)
            crop = px[375 - 352:, 13:13 + 1216] if fmt == "kitti" else px
            want = crop.astype(np.float32) / 255.0                                            # :37-38 / :52-53
        ds = _dataset(str(img_dir), gt_dir, gt_format="cityscapes", image_format=fmt, image_resolution=shape)
        item = ds[0]
        ds.close()
        assert item["img_file_basename"] == ("a" if fmt != "u4k" else "a.raw")  # :70-72 strips .jpg / .png / .jpeg only
        assert torch.equal(item["image_hr"].cpu(), torch.from_numpy(np.ascontiguousarray(want.transpose(2, 0, 1)))), fmt
        assert bit_equal(item["depth_gt"][0, 0].cpu().numpy(), decode_spec(**specs[0])[0])


# ------------------------------------------------------------------------------------------------------------------ end to end
def _write_cfg(tmp_path):
    cfg = tmp_path / "cfg.py"
    cfg.write_text(f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n"
                   f"model = dict(config=dict(patch_process_shape={list(PPS)}, image_raw_shape={list(RAW)}, patch_split_num={list(SPLIT)},\n"
                   "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")
    return str(cfg)


@pytest.fixture(scope="module")
def general_run(tmp_path_factory):
    """a two-frame Cityscapes-format folder at the E2E_V2 case's size, the model the CLI would build for it (synthetic weights), and
    Tester.run with one and two frames per call; ``scored`` records what get_metrics was handed"""
    from patchrefinerv2_amd import models, weights as W  # noqa: F401
    from patchrefinerv2_amd.registry import DATASETS, Config, build_model
    from patchrefinerv2_amd.tester import RunnerInfo, Tester
    tmp = tmp_path_factory.mktemp("general")
    img_dir, gt_dir, specs = write_general_tree(str(tmp / "data"), "cityscapes", RAW, n=2)
    cfg_path = _write_cfg(tmp)
    cfg = Config.fromfile(cfg_path)
    mcfg = cfg.model.to_dict()
    mcfg["config"].update(prec="bf16x3", max_batch=41, n_streams=3)  # tools/test.py's defaults
    model = build_model(mcfg)
    model.load_state_dict(W.synth_state_dict(model.spec(), seed=0), strict=True)
    ds = DATASETS.build(dict(cfg.general_dataloader.dataset.to_dict(), rgb_image_dir=img_dir, gt_dir=gt_dir, gt_format="cityscapes",
                             image_resolution=list(RAW)))
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
    ds.close()
    return dict(tmp=tmp, cfg=cfg_path, img_dir=img_dir, gt_dir=gt_dir, specs=specs, one=one, two=two, scored=scored[:n_one], last_eval=last_eval)


def test_tester_run_metrics_equal_host_compute_metrics(general_run):
    from patchrefinerv2_amd import metrics as M
    one = general_run["one"]
    assert [r["name"] for r in one] == ["frame_000.npy", "frame_001.npy"] and len(general_run["scored"]) == 2
    for r, spec, (gt, result, edges) in zip(one, general_run["specs"], general_run["scored"]):
        assert r["shape"] == (1, 1) + OUT == tuple(result.shape) and tuple(gt.shape) == (1, 1) + RAW  # scoring resizes the map
        want_d, want_b = decode_spec(**spec)
        assert bit_equal(gt[0, 0].numpy(), want_d) and np.array_equal(edges.numpy(), want_b)
        ref = M.compute_metrics(gt, result, disp_gt_edges=want_b, min_depth_eval=1e-3, max_depth_eval=80, garg_crop=False, eigen_crop=False,
                                dataset="")
        _close(r["metrics"], ref, r["name"])
        assert r["metrics"]["see"] > 0 and 0 < r["metrics"]["abs_rel"] < 100
    assert one[0]["metrics"] != one[1]["metrics"]
    ev = general_run["last_eval"]
    assert "see" in ev and ev["see"] == float(np.mean([r["metrics"]["see"] for r in one])) and set(ev) == set(one[0]["metrics"])


def test_frame_batch_two_gives_the_same_dicts(general_run):
    assert [r["metrics"] for r in general_run["two"]] == [r["metrics"] for r in general_run["one"]]
    assert [r["name"] for r in general_run["two"]] == [r["name"] for r in general_run["one"]]


def test_cli_test_type_general_prints_the_metric_table(general_run):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), general_run["cfg"], "--synthetic-weights", "--cai-mode", "m1",
                        "--test-type", "general", "--image-raw-shape", str(RAW[0]), str(RAW[1]), "--patch-split-num", "2", "2", "--cfg-option",
                        "general_dataloader.dataset.gt_format=cityscapes", f"general_dataloader.dataset.gt_dir={general_run['gt_dir']}",
                        f"general_dataloader.dataset.rgb_image_dir={general_run['img_dir']}"],
                       capture_output=True, text=True, timeout=600, cwd=str(general_run["tmp"]))
    assert r.returncode == 0, r.stderr[-2000:]
    for res in general_run["one"]:
        assert f"{res['name']}: depth {(1, 1) + OUT}" in r.stdout
    table = [ln for ln in r.stdout.splitlines() if " see " in ln and "abs_rel" in ln]
    assert len(table) == 1, r.stdout[-2000:]
    printed = {k: float(v) for k, v in (kv.split(" ") for kv in re.sub(r"^\[rank 0\] ", "", table[0]).split(", "))}
    assert set(printed) == set(general_run["last_eval"])
    for k, v in printed.items():
        assert abs(v - general_run["last_eval"][k]) <= 1e-4 * max(1.0, abs(general_run["last_eval"][k])), (k, v)
