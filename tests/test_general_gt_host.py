"""CPU: the general dataset's ground-truth decoders without a GPU -- a numpy restatement of the decode rules (``decode_spec``, the
spec of csrc/evalgt.hip's gt_decode_kernel) against the reference's own DepthMap outputs (tests/golden/general_gt.npz, written by
tools/make_general_gt_golden.py), the host parsing of tester.ImageDataset(gt_format=...), its unchanged defaults, and the two new
entry points through the C ABI."""
import ctypes
import hashlib
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "general_gt.npz")
NEW_SYMBOLS = ("prv2_gt_decode", "prv2_depth_metrics_lowres")
NEW_OPS = ("gt_decode", "depth_metrics_lowres")
CITYSCAPES_FACTOR = np.float32(0.209313 * 2262.52)
ETH_SHAPE = (4032, 6048)


# ------------------------------------------------------------------------------------------------------------------ the spec
def boundaries_spec(e, th=1.0):
    """get_boundaries(e, th, dilation=0) (metric.py:74-85) written out: a pixel is set when |difference| to its upper, lower, left or
    right neighbour exceeds th (float32 differences; a comparison with NaN is false; a frame border has no neighbour) -> uint8"""
    e = np.asarray(e, np.float32)
    th = np.float32(th)
    out = np.zeros(e.shape, bool)
    with np.errstate(invalid="ignore"):
        dy = np.abs(e[1:, :] - e[:-1, :]) > th
        dx = np.abs(e[:, 1:] - e[:, :-1]) > th
    out[1:, :] |= dy
    out[:-1, :] |= dy
    out[:, 1:] |= dx
    out[:, :-1] |= dx
    return out.astype(np.uint8)


def decode_spec(kind, src, factor=None, doffs=None, th=1.0):
    """the decode rules of the four formats on the map as the reference holds it after reading the file (rows top to bottom, host
    byte order) -> (depth float32, boundary uint8).  Every operation is a float32 numpy operation in the reference's order."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kind == "u4k":  # general_dataset.py:88-94
            d = np.asarray(src).astype(np.float32)
            return (np.float32(factor) / d).astype(np.float32), boundaries_spec(d, th)
        if kind == "eth3d":  # :106-111
            v = np.asarray(src, np.float32)
            d = np.where(np.isfinite(v), v, np.float32(0)).astype(np.float32)
            return d, boundaries_spec(d, th)
        if kind == "mid":  # :125-139
            v = np.asarray(src, np.float32)
            inv = v == np.float32(np.inf)
            depth = ((np.float32(factor) / (v + np.float32(doffs))) / np.float32(1000)).astype(np.float32)
            depth[inv] = 0
            e = v.copy()
            e[inv] = 0
            return depth, boundaries_spec(e, th)
        if kind == "cityscapes":  # :142-151
            assert np.asarray(src).dtype == np.uint16
            f = np.asarray(src).astype(np.float32)
            t = np.where(src > 0, (f - np.float32(1)) / np.float32(256), f).astype(np.float32)
            q = (np.float32(CITYSCAPES_FACTOR if factor is None else factor) / t).astype(np.float32)
            depth = np.where(np.isfinite(q), q, np.float32(0)).astype(np.float32)
            return depth, boundaries_spec(depth, th)
    raise ValueError(kind)


def bit_equal(a, b):
    """float32 arrays equal bit for bit outside NaN, NaN at the same positions"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def eth3d_input(shape=ETH_SHAPE):
    """the full-size ETH3D input of tools/make_general_gt_golden.py (integer arithmetic and one float32 scale: the same on every host)"""
    h, w = shape
    y, x = np.arange(h, dtype=np.uint32)[:, None], np.arange(w, dtype=np.uint32)[None, :]
    t = ((x * np.uint32(2654435761) + y * np.uint32(40503)) >> np.uint32(7)) & np.uint32(1023)
    steps = (x // np.uint32(577) + y // np.uint32(811)) % np.uint32(5)
    d = (t.astype(np.float32) * np.float32(1.0 / 2048.0) + steps.astype(np.float32) * np.float32(2.5) + np.float32(1.0)).astype(np.float32)
    k = (x * np.uint32(7919) + y * np.uint32(104729)) % np.uint32(9973)
    d[k == 0] = np.inf
    d[k == 1] = -np.inf
    d[k == 2] = np.nan
    d[(x % np.uint32(1511) < 3) & (y % np.uint32(997) < 2)] = np.inf
    return d


def test_spec_reproduces_the_reference_outputs():
    z = np.load(GOLDEN)
    cases = [str(c) for c in z["cases"]]
    assert sorted(cases) == ["cityscapes", "mid_be", "mid_le", "u4k_a32", "u4k_b64"]
    for c in cases:
        kind = str(z[f"{c}/kind"])
        kw = {k: float(z[f"{c}/{k}"]) for k in ("factor", "doffs") if f"{c}/{k}" in z.files}
        depth, boundary = decode_spec(kind, z[f"{c}/input"], **kw)
        gt, edge = z[f"{c}/gt"], z[f"{c}/edge"]
        assert gt.dtype == np.float32 and bit_equal(depth, gt), c
        assert np.array_equal(boundary, edge.astype(np.uint8)) and set(np.unique(edge)) <= {0.0, 1.0}, c
        assert boundary.sum() > 20, c  # not vacuous
    assert np.isnan(z["u4k_a32/gt"]).sum() == 1 and np.isinf(z["u4k_a32/gt"]).sum() == 1  # disparity NaN / 0 stay NaN / inf
    assert (z["mid_le/gt"] == 0).sum() == 5 and np.isnan(z["mid_le/gt"]).sum() == 1       # four +inf and the -inf (-0.0); NaN stays
    assert np.isinf(z["mid_le/gt"]).sum() == 1                                               # disp == -doffs: a division by zero stays inf
    assert (z["cityscapes/gt"] == 0).sum() >= 8                                              # samples 0 and 1 decode to 0


def test_spec_reproduces_the_eth3d_digests():
    z = np.load(GOLDEN)
    assert tuple(z["eth3d/shape"]) == ETH_SHAPE
    depth, boundary = decode_spec("eth3d", eth3d_input())
    assert bit_equal(depth[:16, :16], z["eth3d/gt_corner"]) and np.array_equal(boundary[:16, :16], z["eth3d/edge_corner"].astype(np.uint8))
    assert int(boundary.sum()) == int(z["eth3d/edge_count"]) and int((depth == 0).sum()) == int(z["eth3d/zero_count"])
    assert hashlib.sha256(depth.tobytes()).hexdigest() == str(z["eth3d/gt_sha256"])
    assert hashlib.sha256(boundary.astype(np.float32).tobytes()).hexdigest() == str(z["eth3d/edge_sha256"])


# ------------------------------------------------------------------------------------------------------------------ synthetic folders
CALIB = "cam0=[3997.684 0 1176.728; 0 3997.684 1011.728; 0 0 1]\ncam1=[3997.684 0 1307.839; 0 3997.684 1011.728; 0 0 1]\n" \
        "doffs=131.111\nbaseline=193.001\nwidth=2964\nheight=1988\nndisp=280\n"


def write_pfm(path, disp, little):
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n%s\n" % (disp.shape[1], disp.shape[0], b"-1.0" if little else b"1.0"))
        f.write(np.flipud(disp).astype("<f4" if little else ">f4").tobytes())


def gt_map(fmt, shape, k):
    """frame k's ground-truth map of format ``fmt`` as the reference would hold it (what decode_spec takes)"""
    h, w = shape
    rs = np.random.RandomState(100 + k)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = 20.0 + 30.0 * (x > w * 0.4 + 3 * k) + 12.0 * (np.hypot(x - w * 0.6, y - h * 0.5) < h * 0.25) + 0.2 * rs.rand(h, w)
    if fmt == "u4k":
        d = base.astype(np.float32)
        d[:2] = 0.0
        return d
    if fmt == "eth3d":  # metric depth with holes
        d = (base / 8.0).astype(np.float32)
        d[:2], d[5, 7], d[4, 6] = np.inf, np.nan, -np.inf
        return d
    if fmt == "mid":  # disparity in pixels of a wide frame; +inf marks the invalid pixels
        d = (base * 4.0).astype(np.float32)
        d[:2], d[5, 7] = np.inf, np.nan
        return d
    v = (base * 100.0).astype(np.uint16)  # cityscapes: uint16 samples, 0 = invalid
    v[:2], v[5, 7] = 0, 1
    return v


def write_general_tree(root, fmt, shape, n=2, image_shape=None):
    """a folder pair as ImageDataset(gt_format=fmt) reads it: images (uint8 .npy, RGB) under <root>/images and the ground truth of
    ``fmt`` with its side files -> (rgb_image_dir, gt_dir, [decode_spec arguments per frame]); file names sort in frame order"""
    from patchrefinerv2_amd.tester import write_png16
    img_dir = os.path.join(root, "images")
    gt_dir = os.path.join(root, {"u4k": "val_gt", "mid": "gts"}.get(fmt, "gt"))
    os.makedirs(img_dir), os.makedirs(gt_dir)
    specs = []
    for k in range(n):
        name = f"frame_{k:03d}"
        rs = np.random.RandomState(k)
        np.save(os.path.join(img_dir, name + ".npy"), rs.randint(0, 256, tuple(image_shape or shape) + (3,)).astype(np.uint8))
        m = gt_map(fmt, shape, k)
        if fmt == "u4k":
            os.makedirs(os.path.join(root, "val_factor"), exist_ok=True)
            np.save(os.path.join(gt_dir, name + ".npy"), m)
            with open(os.path.join(root, "val_factor", name + ".txt"), "w") as f:
                f.write(f"{900.5 + k}\n")
            specs.append(dict(kind="u4k", src=m, factor=900.5 + k))
        elif fmt == "eth3d":
            m.tofile(os.path.join(gt_dir, name + ".raw"))
            specs.append(dict(kind="eth3d", src=m))
        elif fmt == "mid":
            os.makedirs(os.path.join(root, "calibs"), exist_ok=True)
            write_pfm(os.path.join(gt_dir, name + ".pfm"), m, little=k % 2 == 0)  # both byte orders
            with open(os.path.join(root, "calibs", name + ".txt"), "w") as f:
                f.write(CALIB)
            specs.append(dict(kind="mid", src=m, factor=193.001 * 3997.684, doffs=131.111))
        else:
            write_png16(os.path.join(gt_dir, name + ".png"), m)
            specs.append(dict(kind="cityscapes", src=m))
    return img_dir, gt_dir, specs


def _dataset(img_dir, gt_dir=None, **kw):
    from patchrefinerv2_amd import tester  # noqa: F401  (registers the datasets)
    from patchrefinerv2_amd.registry import DATASETS
    return DATASETS.build(dict(type="ImageDataset", rgb_image_dir=img_dir, gt_dir=gt_dir, **kw))


# ------------------------------------------------------------------------------------------------------------------ parsing
def test_factor_and_calibration_files(tmp_path):
    from patchrefinerv2_amd import datasets as T
    p = tmp_path / "f.txt"
    p.write_text("1234.5678\nignored\n")
    assert T.read_factor_file(str(p)) == 1234.5678
    c = tmp_path / "c.txt"
    c.write_text(CALIB)
    factor, doffs = T.read_mid_calib(str(c))
    assert factor == 193.001 * 3997.684 and doffs == 131.111  # baseline x f of cam0=[f ..., by the reference's expressions
    z = np.load(GOLDEN)
    assert str(z["mid_le/calib"]) == CALIB and float(z["mid_le/factor"]) == factor and float(z["mid_le/doffs"]) == doffs


def test_pfm_header(tmp_path):
    from patchrefinerv2_amd import datasets as T
    assert T.read_pfm_header(io.BytesIO(b"Pf\n23 17\n-1.0\nDATA")) == (23, 17, True, 1.0, 14)
    assert T.read_pfm_header(io.BytesIO(b"Pf\n640 480\n0.25\n")) == (640, 480, False, 0.25, 16)
    for bad in (b"P5\n23 17\n-1.0\n", b"PF\n23 17\n-1.0\n", b"Pf\n23x17\n-1.0\n", b"Pf\n23 17 3\n-1.0\n", b"Pf\n23 17\nscale\n", b"Pf\n0 17\n1.0\n",
                b"", b"Pf\n\xff\xfe 17\n1.0\n"):
        with pytest.raises(ValueError, match="PFM"):
            T.read_pfm_header(io.BytesIO(bad))
    # through the dataset: the file's name is in the message, a payload of the wrong size is rejected too
    img_dir, gt_dir, _ = write_general_tree(str(tmp_path / "mid"), "mid", (6, 8))
    ds = _dataset(img_dir, gt_dir, gt_format="mid")
    m0, m1 = ds.gt_meta(0), ds.gt_meta(1)
    host_little = sys.byteorder == "little"
    assert m0["shape"] == m1["shape"] == (6, 8) and m0["nbytes"] == 6 * 8 * 4 and m0["offset"] == len(b"Pf\n8 6\n-1.0\n")
    assert m0["byteswap"] == (not host_little) and m1["byteswap"] == host_little  # frame 0 little-endian, frame 1 big-endian
    assert (m0["factor"], m0["doffs"]) == (193.001 * 3997.684, 131.111)
    with open(os.path.join(gt_dir, "frame_000.pfm"), "wb") as f:
        f.write(b"Pf\n8 6\n-1.0\n" + bytes(6 * 8 * 4 - 4))
    with open(os.path.join(gt_dir, "frame_001.pfm"), "wb") as f:
        f.write(b"Pg\n8 6\n-1.0\n" + bytes(6 * 8 * 4))
    ds = _dataset(img_dir, gt_dir, gt_format="mid")
    with pytest.raises(ValueError, match=r"frame_000\.pfm.*payload"):
        ds.gt_meta(0)
    with pytest.raises(ValueError, match=r"frame_001\.pfm.*Not a PFM"):
        ds.gt_meta(1)


def test_sorted_pairing_count_mismatch_and_names(tmp_path):
    from patchrefinerv2_amd import datasets as T
    from patchrefinerv2_amd.tester import write_png8
    img_dir, gt_dir, _ = write_general_tree(str(tmp_path / "u4k"), "u4k", (6, 8), n=3)
    # the pairing is by sorted position, not by name
    os.rename(os.path.join(gt_dir, "frame_001.npy"), os.path.join(gt_dir, "a_first.npy"))
    os.rename(os.path.join(tmp_path / "u4k" / "val_factor", "frame_001.txt"), os.path.join(tmp_path / "u4k" / "val_factor", "a_first.txt"))
    ds = _dataset(img_dir, gt_dir, gt_format="u4k")
    assert ds.files == ["frame_000.npy", "frame_001.npy", "frame_002.npy"] and ds.gt_files == ["a_first.npy", "frame_000.npy", "frame_002.npy"]
    assert ds.gt_meta(0)["path"] == os.path.join(gt_dir, "a_first.npy") and ds.gt_meta(0)["factor"] == 901.5  # val_gt -> val_factor, .npy -> .txt
    assert ds.gt_meta(1)["factor"] == 900.5 and ds.gt_meta(2)["shape"] == (6, 8)
    os.remove(os.path.join(gt_dir, "frame_002.npy"))
    with pytest.raises(ValueError, match="3 images .* 2 ground-truth files"):
        _dataset(img_dir, gt_dir, gt_format="u4k")
    assert _dataset(img_dir, gt_dir).gt_format is None  # today's convention does not list gt_dir
    # general_dataset.py:70-72 and :156-157
    assert T.strip_image_name("a.png") == "a" and T.strip_image_name("b.jpeg") == "b" and T.strip_image_name("c.jpg.png") == "c"
    assert T.strip_image_name("d.raw") == "d.raw" and T.strip_gt_name("e.npy") == "e" and T.strip_gt_name("f.exr") == "f"
    assert T.strip_gt_name("g.pfm") == "g.pfm"
    z = np.load(GOLDEN)
    for c, name in (("u4k_a32", "a32.npy"), ("mid_le", "le.pfm"), ("cityscapes", "c.png")):
        assert T.strip_gt_name(name) == str(z[f"{c}/name"])
    # eth3d: the file must hold gt_shape float32 samples; cityscapes: a 16-bit greyscale PNG
    img_dir, gt_dir, _ = write_general_tree(str(tmp_path / "eth"), "eth3d", (6, 8))
    assert _dataset(img_dir, gt_dir, gt_format="eth3d", gt_shape=(6, 8)).gt_meta(1)["nbytes"] == 192
    with pytest.raises(ValueError, match="gt_shape"):
        _dataset(img_dir, gt_dir, gt_format="eth3d").gt_meta(0)  # the default 4032 x 6048
    img_dir, gt_dir, _ = write_general_tree(str(tmp_path / "cs"), "cityscapes", (6, 8))
    m = _dataset(img_dir, gt_dir, gt_format="cityscapes").gt_meta(0)
    assert m["shape"] == (6, 8) and m["nbytes"] == 96
    write_png8(os.path.join(gt_dir, "frame_001.png"), np.zeros((6, 8), np.uint8))
    with pytest.raises(ValueError, match="16-bit"):
        _dataset(img_dir, gt_dir, gt_format="cityscapes").gt_meta(1)


def test_kb_crop_and_image_formats(tmp_path):
    from PIL import Image
    from patchrefinerv2_amd import datasets as T
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, (375, 1242, 3)).astype(np.uint8)
    Image.fromarray(img).save(tmp_path / "k.png")
    px, swap = T.decode_image_u8(str(tmp_path / "k.png"), "kitti", None)
    top, left = 375 - 352, int((1242 - 1216) / 2)
    assert not swap and np.array_equal(px, img[top:top + 352, left:left + 1216])
    px, swap = T.decode_image_u8(str(tmp_path / "k.png"), "cityscapes", None)
    assert not swap and np.array_equal(px, img)
    Image.fromarray(img[:300]).save(tmp_path / "small.png")
    with pytest.raises(ValueError, match="smaller than the kb-crop 352 x 1216"):
        T.decode_image_u8(str(tmp_path / "small.png"), "kitti", None)
    img[:6, :8].tofile(tmp_path / "u.raw")
    px, swap = T.decode_image_u8(str(tmp_path / "u.raw"), "u4k", (6, 8))
    assert swap and np.array_equal(px, img[:6, :8])
    with pytest.raises(ValueError, match="expected 150"):
        T.decode_image_u8(str(tmp_path / "u.raw"), "u4k", (5, 10))
    with pytest.raises(ValueError, match="image_format"):
        _dataset(str(tmp_path), image_format="nyu")
    with pytest.raises(ValueError, match="gt_format"):
        _dataset(str(tmp_path), str(tmp_path), gt_format="kitti")


# ------------------------------------------------------------------------------------------------------------------ defaults
def test_default_items_are_unchanged_and_gta_is_not_built(tmp_path, monkeypatch):
    from patchrefinerv2_amd import datasets as T, metrics as M
    img_dir, gt_dir = tmp_path / "img", tmp_path / "gt"
    os.makedirs(img_dir), os.makedirs(gt_dir)
    rs = np.random.RandomState(4)
    gts = {}
    for name in ("b.x", "a"):
        np.save(img_dir / f"{name}.npy", rs.randint(0, 256, (6, 8, 3)).astype(np.uint8))
        gts[name] = (2.0 + 3.0 * (np.mgrid[0:6, 0:8][1] > 3) + rs.rand(6, 8)).astype(np.float64)
        np.save(gt_dir / f"{name}.npy", gts[name])
    seen = []

    def fake_read(path, image_resolution=(2160, 3840), device="cuda"):  # (the bicubic resize needs the GPU)
        seen.append((path, tuple(image_resolution)))
        return torch.full((3, 2, 2), float(len(seen)))
    monkeypatch.setattr(T, "read_image_device", fake_read)
    ds = _dataset(str(img_dir), str(gt_dir), image_resolution=(12, 16))
    assert ds.gt_format is None and ds.image_format is None and len(ds) == 2 and not hasattr(ds, "gt_files")
    for i, name in enumerate(("a", "b.x")):
        item = ds[i]
        assert set(item) == {"image_hr", "img_file_basename", "depth_gt", "boundary"} and item["img_file_basename"] == name  # splitext
        assert seen[-1] == (str(img_dir / f"{name}.npy"), (12, 16)) and torch.equal(item["image_hr"], torch.full((3, 2, 2), float(i + 1)))
        gt = gts[name].astype(np.float32)
        assert item["depth_gt"].dtype == torch.float32 and torch.equal(item["depth_gt"], torch.from_numpy(gt)[None, None])
        assert item["boundary"].dtype == torch.float32 and np.array_equal(item["boundary"].numpy(), M.get_boundaries(gt, th=1, dilation=0))
        assert item["boundary"].sum() > 0
    assert set(_dataset(str(img_dir))[0]) == {"image_hr", "img_file_basename"}
    with pytest.raises(NotImplementedError, match="imageio"):
        _dataset(str(img_dir), str(gt_dir), gt_format="gta")


def test_cfg_option_reaches_the_constructor(tmp_path):
    """tools/test.py: --cfg-option general_dataloader.dataset.gt_format=... needs no new flag"""
    import argparse
    import importlib.util
    from patchrefinerv2_amd.registry import Config
    spec = importlib.util.spec_from_file_location("prv2_tools_test_general", os.path.join(ROOT, "tools", "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    img_dir, gt_dir, _ = write_general_tree(str(tmp_path / "cs"), "cityscapes", (6, 8))
    cfg = Config.fromfile(os.path.join(ROOT, "configs", "v2_dav2_mobile_u4k.py"))
    cfg.merge_from_dict(cli.parse_opts(["general_dataloader.dataset.gt_format=cityscapes", f"general_dataloader.dataset.gt_dir={gt_dir}",
                                        f"general_dataloader.dataset.rgb_image_dir={img_dir}", "general_dataloader.dataset.image_format=cityscapes"]))
    d = cli.dataset_config(cfg, argparse.Namespace(test_type="general", config="cfg.py", image_raw_shape=[6, 8], edge_metrics=False))
    from patchrefinerv2_amd.registry import DATASETS
    ds = DATASETS.build(d)
    assert (ds.gt_format, ds.image_format, ds.gt_dir, ds.image_resolution) == ("cityscapes", "cityscapes", gt_dir, (6, 8))
    assert len(ds.gt_files) == 2
    for kind in ("CityScapesDataset", "KittiDataset", "ScanNetDataset", "ETH3DDataset"):
        assert kind not in DATASETS  # the dataset classes stay unbuilt


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_are_declared_bound_and_exported_on_abi_20():
    from patchrefinerv2_amd import lib as L, ops, torch_ops
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20  # additive: the ABI stays at 20
    raw = ctypes.CDLL(L.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in L.SIGNATURES and re.search(rf"\bint {s}\(", hdr) and hasattr(raw, s), s
    assert L.load().prv2_abi_version() == 20
    # the header's argument lists and the ctypes table agree in length, and each entry cites its reference call site
    for s in NEW_SYMBOLS:
        args = re.search(rf"\bint {s}\((.*?)\);", hdr, flags=re.S).group(1)
        assert len(args.split(",")) == len(L.SIGNATURES[s][1]), s
    assert "general_dataset.py:75-158" in hdr and "metric.py:94-95" in hdr
    kinds = dict(re.findall(r"PRV2_GT_(\w+) = (\d)", hdr))
    assert kinds == {"ETH3D": "0", "MIDDLEBURY": "1", "CITYSCAPES": "2"} and ops.GT_KINDS == {"eth3d": 0, "mid": 1, "cityscapes": 2}
    assert ops.CITYSCAPES_FACTOR == float(CITYSCAPES_FACTOR)
    t = torch_ops.load()
    for o in NEW_OPS:
        assert o in torch_ops.OPS and hasattr(t, o) and hasattr(ops, o)
    f, b = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    for call in (lambda: t.gt_decode(f[0], 0, 1.0, 0.0, 1.0, False, False), lambda: t.depth_metrics_lowres(f, f[:, :4, :4], b, None, 0.1, 10.0, 0, 8, 0, 8)):
        with pytest.raises((RuntimeError, NotImplementedError)):
            call()
    with pytest.raises(ValueError, match="kind"):
        ops.gt_decode(f[0], "gta")
    with pytest.raises(ValueError, match="GPU"):
        ops.gt_decode(f[0], "eth3d")


def test_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    P = 4096  # a non-null address that is never dereferenced: every call below fails its checks first

    def err(code):
        assert code != 0
        return lib.prv2_last_error()

    def gd(src=P, kind=0, h=4, w=4, depth=P, boundary=P):
        return lib.prv2_gt_decode(src, kind, h, w, 2.0, 0.5, 1.0, 0, 0, depth, boundary, None)
    assert b"null" in err(gd(src=None))
    assert b"null" in err(gd(depth=None))
    assert b"null" in err(gd(boundary=None))
    assert b"kind" in err(gd(kind=3))
    assert b"kind" in err(gd(kind=-1))
    assert b"shape" in err(gd(h=0))
    assert b"shape" in err(gd(h=-4))
    assert b"shape" in err(gd(w=0))
    assert b"2^31" in err(gd(h=65536, w=32768))
    ws = lib.prv2_depth_metrics_workspace_bytes(2, 16, 24)

    def dm(gt=P, pred=P, n=2, h=16, w=24, ph=8, pw=12, crop=(0, 16, 0, 24), sums=P, wsp=P, wsb=ws):
        return lib.prv2_depth_metrics_lowres(gt, pred, None, None, n, h, w, ph, pw, 0.1, 10.0, *crop, sums, wsp, wsb, None)
    assert b"null" in err(dm(gt=None))
    assert b"null" in err(dm(pred=None))
    assert b"null" in err(dm(sums=None))
    assert b"workspace" in err(dm(wsp=None))
    assert b"workspace" in err(dm(wsb=ws - 1))
    assert b"frame count" in err(dm(n=0))
    assert b"shape" in err(dm(h=0))
    assert b"shape" in err(dm(h=-1))
    assert b"prediction shape" in err(dm(ph=0))
    assert b"prediction shape" in err(dm(pw=-2))
    assert b"crop" in err(dm(crop=(0, 17, 0, 24)))
    assert b"crop" in err(dm(crop=(0, 16, 5, 4)))
    assert b"depth_metrics_lowres" in lib.prv2_last_error()
