"""CPU: ETHDataset without a GPU -- the specification of its device work and the host half of the class.

``edge_region_torch`` restates eth_dataset.py:261-272 with torch ops (kornia is not installed).  The result depends on kornia only through
these properties, which the restatement keeps: ``spatial_gradient`` is the Sobel pair up to scale and sign (the magnitude is compared with
a fraction of its own maximum), its padding is replicate, ``gaussian_blur2d``'s weights are positive and its border is reflect.  The
specification (``edge_region_spec``) runs the gradient and the threshold in float64 and the two steps after them (blur, resize) in float32
with torch's own CPU ops, as the reference does (:269-271).  ``edge_region_taps`` is the integer restatement of those two steps that
csrc/evalgt.hip implements; it is checked against them here.  The test images have no pixel whose gradient is within 1e-5 x max of the
threshold (asserted below), so a float32 gradient decides every pixel as float64 does and the GPU's mask can be compared exactly.
``u8_resize_spec`` is the float32 restatement of prv2_u8_image_resize (no contraction).  The GPU file imports all of this."""
import argparse
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("prv2_u8_image_resize", "prv2_image_edge_region_workspace_bytes", "prv2_image_edge_region")
NEW_OPS = ("u8_image_resize", "image_edge_region")
KEYS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel", "see")
KEYS30 = tuple(pre + k for pre in ("edge_", "noedge_", "") for k in KEYS)  # eth_dataset.py:304-335

# image -> ground truth shapes of the edge-area checks
REGION_CASES = [((1, 1), (3, 2)),          # one pixel, scale 0, everything edge
                ((2, 3), (2, 3)),          # every output lands on a source pixel: the upper taps weigh 0
                ((5, 7), (9, 13)),         # scale exactly 0.5: every second output lands exact
                ((37, 53), (70, 99)),      # scalar tails
                ((12, 20), (7, 11)),       # ground truth smaller than the image
                ((135, 240), (252, 448))]  # ETH3D's 28 / 15 ratio over many blocks
# source -> output shapes of the image stage (identity, up, down, a one-row source, the issue's odd pair)
RESIZE_CASES = [((37, 53), (37, 53)), ((37, 53), (70, 99)), ((135, 240), (64, 112)), ((1, 9), (5, 17)), ((63, 95), (34, 51))]
# the largest |u8_resize_spec - F.interpolate (torch CPU)| over RESIZE_CASES, measured by test_u8_resize_spec_against_torch_cpu: torch's own
# kernels contract a * b + c to fused multiply-adds (CPU and device), prv2_u8_image_resize does not; values are in [0, 1], one float32
# ulp below 1 is 5.96e-8
RESIZE_MEASURED_MAX_ABS = 1.8e-7  # 1.788e-7 at (63, 95) -> (34, 51); 1.192e-7 on the upsampling cases; 0 at identity and for one row
RESIZE_ATOL = 4 * RESIZE_MEASURED_MAX_ABS


# ------------------------------------------------------------------------------------------------------------------ the spec
def scene(h, w, seed=1):
    """[3, h, w] float32 in [0, 1]: seeded smooth noise (a bilinear upsample of torch.rand) plus one strong and one weaker step"""
    g = torch.Generator().manual_seed(seed * 100003 + h * 1009 + w)
    base = F.interpolate(torch.rand(1, 3, h // 8 + 2, w // 8 + 2, generator=g), size=(h, w), mode="bilinear", align_corners=True) * 0.5
    base[:, :, h // 3:, w // 2:] += 0.4
    base[:, :, :h // 4, :w // 5] += 0.2
    return base.clamp(0, 1)[0].contiguous()


def scene_u8(h, w, seed=1):
    """``scene`` as the bytes of a photograph, uint8 [h, w, 3]"""
    return (scene(h, w, seed) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy()


def gradient_sum(image, dtype=torch.float64):
    """eth_dataset.py:261-263: kornia.filters.spatial_gradient (mode='sobel', order=1, normalized: kernel / 8, replicate padding) written
    as shifted differences (elementwise torch ops on the image's device: no convolution library), the magnitude per channel, summed
    over the channels -> [h, w]"""
    x = torch.as_tensor(image).to(dtype)
    x = x[0] if x.dim() == 4 else x
    p = F.pad(x[None], (1, 1, 1, 1), mode="replicate")[0]
    u, c, d = p[:, :-2], p[:, 1:-1], p[:, 2:]   # the rows above, at and below
    gx = ((u[:, :, 2:] - u[:, :, :-2]) + 2 * (c[:, :, 2:] - c[:, :, :-2]) + (d[:, :, 2:] - d[:, :, :-2])) / 8
    gy = ((d[:, :, :-2] - u[:, :, :-2]) + 2 * (d[:, :, 1:-1] - u[:, :, 1:-1]) + (d[:, :, 2:] - u[:, :, 2:])) / 8
    m = (gx ** 2 + gy ** 2) ** (1 / 2)
    return m.sum(dim=0)


def blur3(edge):
    """eth_dataset.py:270: kornia.filters.gaussian_blur2d(kernel_size=(3, 3), sigma=(3, 3), border_type='reflect', separable=True) of a
    float32 map [1, 1, h, w], as shifted sums.  Reflect needs two pixels: an axis of one pixel has nothing to reflect and keeps its value."""
    x = torch.arange(3, dtype=torch.float32, device=edge.device) - 1
    g = torch.exp(-x ** 2 / (2 * 3.0 * 3.0))
    g = g / g.sum()
    h, w = edge.shape[-2:]
    if w > 1:
        p = F.pad(edge, (1, 1, 0, 0), mode="reflect")
        edge = g[0] * p[..., :-2] + g[1] * p[..., 1:-1] + g[2] * p[..., 2:]
    if h > 1:
        p = F.pad(edge, (0, 0, 1, 1), mode="reflect")
        edge = g[0] * p[..., :-2, :] + g[1] * p[..., 1:-1, :] + g[2] * p[..., 2:, :]
    return edge


def edge_region_torch(image, H, W, frac=0.5, dtype=torch.float32):
    """eth_dataset.py:261-272 with torch ops on ``image``'s device, the gradient in ``dtype`` -> bool [H, W]"""
    g = gradient_sum(image, dtype)
    edge = g >= g.max() * frac                                                                         # :264-265
    wide = blur3(edge.float()[None, None])                                                             # :269-270
    return (F.interpolate(wide, size=(H, W), mode="bilinear", align_corners=True) > 0)[0, 0]           # :271-272


def edge_region_spec(image, H, W, frac=0.5):
    """the specification: the gradient and its threshold in float64 on the CPU -> uint8 [H, W]"""
    return edge_region_torch(torch.as_tensor(image).cpu(), H, W, frac, torch.float64).numpy().astype(np.uint8)


def ac_taps(n, N):
    """PyTorch's float32 source taps of bilinear(align_corners=True), n -> N: (i0, i1, lambda0, lambda1)"""
    sc = np.float32(n - 1) / np.float32(N - 1) if N > 1 else np.float32(0)
    src = (sc * np.arange(N, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1) - l1).astype(np.float32), l1


def edge_region_taps(edge, H, W):
    """the integer restatement of :270-272 on a bool map [h, w]: 3 x 3 dilation with the window clipped at the frame, then "one of the
    up to four source taps with a non-zero weight is set" -> uint8 [H, W]"""
    e = np.asarray(edge, bool)
    h, w = e.shape
    p = np.zeros((h + 2, w + 2), bool)
    p[1:-1, 1:-1] = e
    d = np.zeros_like(e)
    for dy in range(3):
        for dx in range(3):
            d |= p[dy:dy + h, dx:dx + w]
    y0, y1, _, ly = ac_taps(h, H)
    x0, x1, _, lx = ac_taps(w, W)
    up, right = (ly > 0)[:, None], (lx > 0)[None, :]
    m = d[y0][:, x0] | (d[y0][:, x1] & right) | (d[y1][:, x0] & up) | (d[y1][:, x1] & up & right)
    return m.astype(np.uint8)


def u8_resize_spec(x, H, W):
    """include/prv2.h prv2_u8_image_resize on uint8 [h, w, 3] -> float32 [3, H, W]: every operation a float32 numpy operation"""
    v = (x.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
    y0, y1, ly0, ly1 = ac_taps(x.shape[0], H)
    x0, x1, lx0, lx1 = ac_taps(x.shape[1], W)
    top = (lx0 * v[:, y0][:, :, x0] + lx1 * v[:, y0][:, :, x1]).astype(np.float32)
    bot = (lx0 * v[:, y1][:, :, x0] + lx1 * v[:, y1][:, :, x1]).astype(np.float32)
    return (ly0[None, :, None] * top + ly1[None, :, None] * bot).astype(np.float32)


def u8_resize_torch(x, H, W):
    """eth_dataset.py:150-161 on torch's CPU"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    return F.interpolate(t.permute(2, 0, 1)[None].float() / 255, (H, W), mode="bilinear", align_corners=True)[0].contiguous().numpy()


def resize_source(shape, seed=0):
    """uint8 [h, w, 3] noise holding every byte value when it is large enough"""
    x = np.random.RandomState(seed + shape[0] * 1000 + shape[1]).randint(0, 256, shape + (3,)).astype(np.uint8)
    if x.size >= 256:
        x.reshape(-1)[:256] = np.arange(256)
    return x


def raw_depth(shape, seed):
    """a raw ETH3D depth map: two planes with a step, noise, and NaN / +inf / -inf / 0 samples"""
    h, w = shape
    rs = np.random.RandomState(seed)
    d = (2.0 + 3.0 * (np.arange(w)[None, :] > w * 0.4) + 1.5 * (np.arange(h)[:, None] > h * 0.6) + 0.3 * rs.rand(h, w)).astype(np.float32)
    f = d.reshape(-1)
    idx = rs.permutation(h * w)
    n = max(1, h * w // 40)
    f[idx[:n]], f[idx[n:2 * n]], f[idx[2 * n:3 * n]], f[idx[3 * n:4 * n]] = np.nan, np.inf, -np.inf, 0.0
    return d


def write_eth_tree(root, n, img_shape, gt_shape, seed=3, names=None):
    """a synthetic ETH3D tree: PNG photographs, raw float32 ground truth of another aspect, and a split file of absolute paths written in
    REVERSE order (the dataset sorts by image path) -> (split path, [dict(img, gt, pixels uint8 [h, w, 3], depth raw float32)] sorted)"""
    from PIL import Image
    os.makedirs(os.path.join(root, "scene", "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "scene", "depth"), exist_ok=True)
    items = []
    for i in range(n):
        name = names[i] if names else f"DSC_{i:04d}"
        img, gt = os.path.join(root, "scene", "images", name + ".png"), os.path.join(root, "scene", "depth", name + ".JPG")
        px, d = scene_u8(*img_shape, seed=seed + i), raw_depth(gt_shape, seed + i)
        Image.fromarray(px).save(img)
        d.tofile(gt)
        items.append(dict(img=img, gt=gt, pixels=px, depth=d))
    split = os.path.join(root, "split.txt")
    with open(split, "w") as f:
        for it in reversed(items):
            f.write(f"{it['img']} {it['gt']}\n")
    return split, sorted(items, key=lambda it: it["img"])


def _dataset(split, **kw):
    from patchrefinerv2_amd import tester  # noqa: F401
    from patchrefinerv2_amd.registry import DATASETS
    cfg = dict(type="ETHDataset", mode="infer", split=split, transform_cfg=dict(input_size_deep=[448, 448]), min_depth=1e-3, max_depth=80)
    cfg.update(kw)
    return DATASETS.build(cfg)


# ------------------------------------------------------------------------------------------------------------------ spec tests
# the synthetic tree of the dataset / CLI tests on the GPU: photographs of ETH_PHOTO resized to the E2E_V2 case's frame (ETH_RAW, the
# smallest V2 case the end-to-end GPU tests use), ground truth of another aspect
ETH_PHOTO, ETH_RAW, ETH_GT, ETH_SEED, ETH_FRAMES = (150, 290), (256, 512), (270, 500), 3, 2


def dataset_image(i):
    """the ``image_hr`` of frame ``i`` of that tree by the spec: float32 [3, *ETH_RAW]"""
    return torch.from_numpy(u8_resize_spec(scene_u8(*ETH_PHOTO, seed=ETH_SEED + i), *ETH_RAW))


def region_test_images():
    """every image an exact mask comparison on the GPU is made on"""
    out = [(f"scene{shape}", scene(*shape)) for shape, _ in REGION_CASES]
    out += [(f"constant-plus-pixel{shape} at ({y}, {x})", one_pixel_image(shape, y, x)) for shape, _, y, x in ONE_PIXEL_CASES]
    return out + [(f"dataset frame {i}", dataset_image(i)) for i in range(ETH_FRAMES)]


# (image shape, ground-truth shape, y, x): a single bright pixel in each corner, on each border and inside -- its gradient ring dilates
# inside the frame only; rows at scale exactly 0.5, columns at 13 / 29; and two corners at (5, 7) -> (9, 13), where the scenes' masks are full
ONE_PIXEL_CASES = [((9, 14), (17, 30), y, x) for y, x in ((0, 0), (0, 13), (8, 0), (8, 13), (0, 6), (8, 7), (4, 0), (3, 13), (4, 6))]
ONE_PIXEL_CASES += [((5, 7), (9, 13), 0, 0), ((5, 7), (9, 13), 4, 6)]


def one_pixel_image(shape, y, x):
    img = torch.full((3,) + tuple(shape), 0.25)
    img[:, y, x] = 0.75
    return img


FRACTION_CASES = (0.25, 0.75)  # other thresholds, on scene(37, 53) -> (70, 99)


def test_no_test_image_has_a_pixel_near_the_threshold():
    """the condition of exact mask equality: no pixel with |g - 0.5 max| <= 1e-5 max, and the float32 gradient decides as float64"""
    img = scene(37, 53)
    for frac in FRACTION_CASES:
        g64 = gradient_sum(img)
        assert not ((g64 - frac * g64.max()).abs() <= 1e-5 * g64.max()).any(), frac
    for name, img in region_test_images():
        g64, g32 = gradient_sum(img, torch.float64), gradient_sum(img, torch.float32)
        mx = float(g64.max())
        if mx == 0.0:  # (the one-pixel image) every tap reads the same value: the kernel's differences are exactly 0 and every pixel is
            assert img.numel() == 3, name  # an edge (g >= 0); one pixel is an edge whatever rounding a convolution leaves in g
            continue
        band = (g64 - 0.5 * mx).abs() <= 1e-5 * mx
        print(f"{name}: in band {int(band.sum())}, max |g32 - g64| / max = {float((g32.double() - g64).abs().max()) / mx:.2e}, "
              f"edge share {float((g64 >= 0.5 * mx).float().mean()):.4f}")
        assert not band.any(), name
        assert float((g32.double() - g64).abs().max()) <= 1e-6 * mx, name
        assert torch.equal(g32 >= g32.max() * 0.5, g64 >= g64.max() * 0.5), name


@pytest.mark.parametrize("img_shape,gt_shape", REGION_CASES)
def test_integer_restatement_equals_blur_and_interpolate(img_shape, gt_shape):
    """what the kernels compute after the threshold (dilation, non-zero taps) against torch's own float32 blur + F.interpolate"""
    img = scene(*img_shape)
    g = gradient_sum(img)
    edge = g >= g.max() * 0.5
    want = edge_region_spec(img, *gt_shape)
    assert np.array_equal(edge_region_taps(edge.numpy(), *gt_shape), want)
    if min(img_shape) >= 12:
        assert 0 < want.mean() < 1  # both sets are in play (the masks of the tiny scenes are full: ONE_PIXEL_CASES are sparse there)
    rs = np.random.RandomState(img_shape[0])
    for dens in (0.02, 0.2):  # arbitrary edge maps, corners and borders included
        e = rs.rand(*img_shape) < dens
        e[0, 0] = e[-1, -1] = True
        ref = (F.interpolate(blur3(torch.from_numpy(e).float()[None, None]), size=gt_shape, mode="bilinear", align_corners=True) > 0)[0, 0]
        assert np.array_equal(edge_region_taps(e, *gt_shape), ref.numpy().astype(np.uint8)), (img_shape, gt_shape, dens)


def test_exact_landings_do_not_see_the_next_pixel():
    """(5, 7) -> (9, 13): scale exactly 0.5.  An edge at source (2, 3) alone is dilated to source rows 1 .. 3 x columns 2 .. 4; the
    outputs with a non-zero tap in them are rows 1 .. 7 x columns 3 .. 9: output row 0 lands exactly on source row 0 and does not see
    source row 1, output column 2 lands on source column 1 and does not see column 2"""
    e = np.zeros((5, 7), bool)
    e[2, 3] = True
    m = edge_region_taps(e, 9, 13)
    want = np.zeros((9, 13), np.uint8)
    want[1:8, 3:10] = 1
    assert np.array_equal(m, want)
    ref = (F.interpolate(blur3(torch.from_numpy(e).float()[None, None]), size=(9, 13), mode="bilinear", align_corners=True) > 0)[0, 0]
    assert np.array_equal(ref.numpy().astype(np.uint8), want)


@pytest.mark.parametrize("shape,gt_shape,y,x", ONE_PIXEL_CASES)
def test_one_pixel_dilates_inside_the_frame_only(shape, gt_shape, y, x):
    img = one_pixel_image(shape, y, x)
    g = gradient_sum(img)
    want = edge_region_spec(img, *gt_shape)
    assert np.array_equal(edge_region_taps((g >= g.max() * 0.5).numpy(), *gt_shape), want) and 0 < want.mean() < 1


def test_constant_image_is_all_edge():
    img = torch.full((3, 6, 9), 0.25)
    assert edge_region_spec(img, 11, 4).all() and edge_region_taps(np.ones((6, 9), bool), 11, 4).all()


@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_u8_resize_spec_against_torch_cpu(src, dst):
    x = resize_source(src)
    spec, ref = u8_resize_spec(x, *dst), u8_resize_torch(x, *dst)
    diff = float(np.abs(spec - ref).max())
    print(f"{src}->{dst}: max |spec - torch CPU| = {diff:.3e}")
    assert spec.shape == ref.shape == (3,) + dst
    assert diff <= RESIZE_MEASURED_MAX_ABS  # the measurement the GPU test's tolerance is four times of
    if src == dst:
        assert np.array_equal(spec, (x.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))  # identity: u8_image's bits


# ------------------------------------------------------------------------------------------------------------------ the class
def test_eth_dataset_is_registered():
    from patchrefinerv2_amd import tester
    from patchrefinerv2_amd.registry import DATASETS
    assert "ETHDataset" in DATASETS and tester.ETHDataset.dataset_name == "eth3d"


def test_split_file_parsing_sorting_and_basename(tmp_path):
    split, items = write_eth_tree(str(tmp_path), 3, (12, 20), (7, 11), names=["b_02", "a_10", "c_01"])
    ds = _dataset(split, gt_shape=(7, 11), overlap=270, crop_strategy="16patches", stitcher_stage=1)
    assert len(ds) == 3 and [os.path.basename(i["img_path"]) for i in ds.data_infos] == ["a_10.png", "b_02.png", "c_01.png"]
    for info, it in zip(ds.data_infos, items):
        assert info["img_path"] == it["img"] and info["depth_map_path"] == it["gt"]
        assert info["img_file_basename"] == os.path.splitext(it["img"])[0].replace("/", "_")[1:]  # eth_dataset.py:238-239
        assert not info["img_file_basename"].startswith("_") and info["img_file_basename"].endswith(os.path.basename(it["img"])[:-4])
    assert (ds.overlap, ds.crop_strategy, ds.stitcher_stage, ds.gt_shape, ds.input_size_shallow) == (270, "16patches", 1, (7, 11), None)
    assert (ds.min_depth, ds.max_depth, ds.mode) == (1e-3, 80, "infer")
    assert _dataset(split, transform_cfg=dict(input_size_deep=[448, 448], input_size_shallow=[2160, 3840])).input_size_shallow == (2160, 3840)
    assert _dataset(split).gt_shape == (4032, 6048)  # the reference's literal is the default


def test_wrong_ground_truth_size_names_the_file(tmp_path):
    split, items = write_eth_tree(str(tmp_path), 2, (12, 20), (7, 11))
    ds = _dataset(split, gt_shape=(7, 11))
    assert ds.check_gt_file(0) == items[0]["gt"]
    with open(items[1]["gt"], "ab") as f:
        f.write(b"\0\0\0\0")
    with pytest.raises(ValueError, match=re.escape(items[1]["gt"]) + r": 312 bytes, expected 308 \(7 x 11 float32"):
        ds.check_gt_file(1)
    with pytest.raises(ValueError, match=re.escape(items[0]["gt"])):
        _dataset(split, gt_shape=(8, 11)).check_gt_file(0)


def test_unbuilt_modes_raise(tmp_path):
    split, _ = write_eth_tree(str(tmp_path), 1, (12, 20), (7, 11))
    with pytest.raises(NotImplementedError, match="train"):
        _dataset(split, mode="train")
    with pytest.raises(NotImplementedError, match="random_crop"):
        _dataset(split, transform_cfg=dict(input_size_deep=[448, 448], random_crop=True, random_crop_size=[540, 960]))
    with pytest.raises(NotImplementedError):
        _dataset(split, resize_mode="bicubic")
    with pytest.raises(NotImplementedError):
        _dataset(None)


def test_key_order_and_missing_image(tmp_path):
    from patchrefinerv2_amd import datasets
    split, _ = write_eth_tree(str(tmp_path), 1, (12, 20), (7, 11))
    ds = _dataset(split, gt_shape=(7, 11))
    with pytest.raises(ValueError, match="image_hr"):
        ds.get_metrics(torch.zeros(1, 1, 7, 11), torch.zeros(1, 1, 7, 11), torch.zeros(7, 11))
    fused = {pre + k: float(i) for i, (pre, k) in enumerate((pre, k) for pre in ("", "edge_", "noedge_") for k in KEYS)}  # compute_metrics_fused's order
    ordered = datasets.eth_metric_order(fused)
    assert tuple(ordered) == KEYS30 and ordered == fused and datasets.ETH_METRIC_KEYS == KEYS


def test_evaluate_is_the_nanmean(tmp_path):
    split, _ = write_eth_tree(str(tmp_path), 1, (12, 20), (7, 11))
    ds = _dataset(split, gt_shape=(7, 11))
    nan = float("nan")
    rows = [{k: 1.0 + i for i, k in enumerate(KEYS30)}, {k: 3.0 + i for i, k in enumerate(KEYS30)}, {k: 8.0 + i for i, k in enumerate(KEYS30)}]
    for k in KEYS:
        rows[1]["noedge_" + k] = nan  # a constant image: its no-edge set is empty
    for r in rows:
        r["edge_see"] = nan          # a key that is NaN in every frame stays NaN, without a warning
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ev = ds.evaluate(rows)
    assert tuple(ev) == KEYS30 and all(isinstance(v, float) for v in ev.values())
    for i, k in enumerate(KEYS30):
        if k == "edge_see":
            assert np.isnan(ev[k])
        elif k.startswith("noedge_"):
            assert ev[k] == (1.0 + i + 8.0 + i) / 2  # the NaN frame is left out, not averaged in
        else:
            assert ev[k] == pytest.approx((1.0 + 3.0 + 8.0) / 3 + i)
        if k != "edge_see":
            assert ev[k] == float(np.nanmean([r[k] for r in rows]))


def _cli():
    spec = importlib.util.spec_from_file_location("prv2_tools_test_eth", os.path.join(ROOT, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def eth_config_text(split, gt_shape, shallow, extra=""):
    """the project's small config with an ETHDataset as its val_dataloader"""
    return (f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n{extra}"
            f"val_dataloader = dict(_delete_=True, batch_size=1, num_workers=2, dataset=dict(type='ETHDataset', mode='infer', split={split!r}, "
            f"min_depth=1e-3, max_depth=80, resize_mode='depth-anything', gt_shape={list(gt_shape)}, "
            f"transform_cfg=dict(input_size_deep=[448, 448], input_size_shallow={list(shallow)})))\n")


def test_cli_dataset_config_accepts_eth_dataset(tmp_path):
    from patchrefinerv2_amd.registry import DATASETS, Config
    cli = _cli()
    split, _ = write_eth_tree(str(tmp_path / "data"), 2, (12, 20), (7, 11))
    cfg_path = tmp_path / "cfg.py"
    cfg_path.write_text(eth_config_text(split, (7, 11), (24, 40)))
    cfg = Config.fromfile(str(cfg_path))
    d = cli.dataset_config(cfg, argparse.Namespace(test_type="normal", config=str(cfg_path), image_raw_shape=[24, 40], edge_metrics=True))
    assert d["type"] == "ETHDataset" and "image_resolution" not in d and "image_raw_shape" not in d and "edge_metrics" not in d
    ds = DATASETS.build(d)
    assert len(ds) == 2 and ds.gt_shape == (7, 11) and ds.input_size_shallow == (24, 40) and ds.resize_mode == "depth-anything"


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_are_declared_bound_and_exported_on_abi_20():
    from patchrefinerv2_amd import lib as L, ops, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20  # additive: the ABI stays at 20
    raw = ctypes.CDLL(L.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in L.SIGNATURES and re.search(rf"\bint(?:64_t)? {s}\(", hdr) and hasattr(raw, s), s
        args = re.search(rf"\bint(?:64_t)? {s}\((.*?)\);", hdr, flags=re.S).group(1)
        assert len(args.split(",")) == len(L.SIGNATURES[s][1]), s
    assert "eth_dataset.py:133,150-161" in hdr and "eth_dataset.py:261-272" in hdr  # each entry cites its reference lines
    assert L.load().prv2_abi_version() == 20
    t = torch_ops.load()
    for o in NEW_OPS:
        assert o in torch_ops.OPS and hasattr(t, o) and hasattr(ops, o)
    for call in (lambda: t.u8_image_resize(torch.zeros(4, 4, 3, dtype=torch.uint8), 8, 8), lambda: t.image_edge_region(torch.zeros(3, 4, 4), 8, 8, 0.5)):
        with pytest.raises((RuntimeError, NotImplementedError)):
            call()
    with pytest.raises(ValueError, match="GPU"):
        ops.u8_image_resize(torch.zeros(4, 4, 3, dtype=torch.uint8), 8, 8)
    with pytest.raises(ValueError, match="GPU"):
        ops.image_edge_region(torch.zeros(3, 4, 4), 8, 8)


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    P = 4096  # a non-null, 16-byte aligned address that is never dereferenced: every call below fails its checks first

    def err(code):
        assert code != 0
        return lib.prv2_last_error()

    def rs(src=P, h=4, w=4, dst=P, H=8, W=8):
        return lib.prv2_u8_image_resize(src, h, w, dst, H, W, None)
    assert b"null" in err(rs(src=None))
    assert b"null" in err(rs(dst=None))
    for kw in (dict(h=0), dict(w=-1), dict(H=0), dict(W=-3)):
        assert b"shape" in err(rs(**kw))
    assert b"2^31" in err(rs(h=32768, w=32768))
    assert b"2^31" in err(rs(H=32768, W=32768))
    assert b"u8_image_resize" in lib.prv2_last_error()

    assert lib.prv2_image_edge_region_workspace_bytes(0, 4) == -1 and lib.prv2_image_edge_region_workspace_bytes(4, -1) == -1
    assert lib.prv2_image_edge_region_workspace_bytes(65536, 32768) == -1
    ws = lib.prv2_image_edge_region_workspace_bytes(5, 7)
    assert ws >= 16 + 5 * 7 * 4 + 5 * 7 and ws % 16 == 0

    def er(img=P, h=5, w=7, frac=0.5, region=P, H=9, W=13, wsp=P, wsb=ws):
        return lib.prv2_image_edge_region(img, h, w, frac, region, H, W, wsp, wsb, None)
    assert b"null" in err(er(img=None))
    assert b"null" in err(er(region=None))
    assert b"image shape" in err(er(h=0))
    assert b"region shape" in err(er(W=0))
    assert b"2^31" in err(er(H=65536, W=32768))
    assert b"NaN" in err(er(frac=float("nan")))
    assert b"workspace" in err(er(wsp=None))
    assert b"workspace" in err(er(wsp=P + 4))
    assert b"workspace" in err(er(wsb=ws - 1))
    assert b"image_edge_region" in lib.prv2_last_error()
