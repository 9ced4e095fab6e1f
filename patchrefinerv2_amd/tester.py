"""Inference driver + general image dataset (the callers on either side of the hot path).

Tester.run          estimator/tester/tester.py:52-127 (frame loop, model call contract, uint16 PNG x256)
Tester.generate_pl  estimator/tester/tester.py:132-181 (pseudo labels: depth, uncertainty and tile-count PNGs)
ImageDataset        estimator/datasets/general_dataset.py:64-245 (folder of images -> image_hr / image_lr; with ``gt_format`` the
                    ground truth of a u4k / eth3d / mid / cityscapes folder, decoded on the GPU -> depth_gt / boundary)
UnrealStereo4kDataset  estimator/datasets/u4k_dataset.py:20-233 (split file -> image_hr / depth_gt / boundary, decoded on the GPU)
ETHDataset          estimator/datasets/eth_dataset.py:23-385 (split file -> image_hr resized on the GPU / depth_gt / boundary; every
                    metric also inside and outside the image's edge area, found on the GPU)
``ssi_metrics=True`` (tools/test.py --ssi-metrics) on any of the three datasets: get_metrics adds the scale-and-shift-invariant scores
                    of estimator/models/losses.py:523-544, :600-700 (metrics.SSI_KEYS; two fused GPU passes, csrc/ssi_eval.hip)
read_image          estimator/datasets/general_dataset.py:22-62 (RGB/255 -> bicubic, align_corners=True)
``runner_info.device_output`` (tools/test.py --device-output) routes the saved files through output.OutputStage: scanlines made on
the GPU, deflate on a writer pool; the default is the host route below.  ``runner_info.device_deflate`` (--device-deflate, needs
device_output) makes the zlib streams on the GPU as well: the files hold the device route's pixels, but not its bytes (the deflate
stream differs from zlib's).
With ``--save``: <name>.png (colour map, tester.py:72-87), <name>_uint16.png (depth x 256, :89-91), <name>_coarse.png
(coarse prediction resized to the raw shape, :93-96) and <name>_edge.png (Canny edges of the log depth, widened by one pixel,
:98-106; metrics.depth_edges) -- colour maps and metrics in metrics.py, PNGs through a dependency-free encoder.  Not built: the
``gta`` ground truth (general_dataset.py:96-101: .exr files need imageio, which is absent) and the dataset classes KittiDataset,
ScanNetDataset and CityScapesDataset; of the reference's dataset classes UnrealStereo4kDataset and ETHDataset are.  Without
``gt_format`` ground truth is metric depth as <basename>.npy files.
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from .registry import DATASETS


def write_png16(path: str, arr_u16: np.ndarray):
    """Minimal PNG encoder: 16-bit grayscale (== PIL's Image.fromarray(uint16).save)."""
    assert arr_u16.dtype == np.uint16 and arr_u16.ndim == 2
    h, w = arr_u16.shape
    raw = np.zeros((h, 1 + 2 * w), dtype=np.uint8)  # filter byte 0 per scanline
    raw[:, 1:] = arr_u16.astype(">u2").view(np.uint8).reshape(h, 2 * w)

    def chunk(tag, data):
        c = struct.pack(">I", len(data)) + tag + data
        return c + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 0, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)))
        f.write(chunk(b"IEND", b""))


def write_png8(path: str, arr_u8: np.ndarray):
    """8-bit RGB / RGBA / gray PNG (== cv2.imwrite of the BGR-swapped array the reference builds)."""
    assert arr_u8.dtype == np.uint8 and arr_u8.ndim in (2, 3)
    h, w = arr_u8.shape[:2]
    ch = 1 if arr_u8.ndim == 2 else arr_u8.shape[2]
    ctype = {1: 0, 3: 2, 4: 6}[ch]
    raw = np.zeros((h, 1 + w * ch), dtype=np.uint8)
    raw[:, 1:] = arr_u8.reshape(h, w * ch)

    def chunk(tag, data):
        c = struct.pack(">I", len(data)) + tag + data
        return c + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw.tobytes(), 6)))
        f.write(chunk(b"IEND", b""))


def read_image_device(path, image_resolution=(2160, 3840), device="cuda") -> torch.Tensor:
    """general_dataset.py:22-62, generic branch, with the resize on the GPU: decode (host), H2D of the SOURCE image (a few MB
    instead of the 99.5 MB 4K frame), RGB/255 + bicubic(align_corners=True) by prv2_bicubic_resize -> [3, H, W] fp32 on device."""
    from . import ops
    if path.endswith(".npy"):
        a = np.load(path)
        img = torch.from_numpy(a.astype(np.float32) / (255.0 if a.max() > 1.5 else 1.0)) if a.dtype != np.uint8 else torch.from_numpy(a)
    else:
        try:
            from PIL import Image
        except ImportError as e:  # pragma: no cover
            raise RuntimeError("PIL is needed to decode image files (or pass .npy arrays)") from e
        img = torch.from_numpy(np.asarray(Image.open(path).convert("RGB")).copy())
    return ops.bicubic_resize(img.to(device), int(image_resolution[0]), int(image_resolution[1]))


def read_image(path, dataset_name="", image_resolution=(2160, 3840)) -> np.ndarray:
    """general_dataset.py:22-62, generic branch on the host (torch CPU): decode, RGB/255, bicubic(align_corners=True)."""
    if path.endswith(".npy"):
        img = np.load(path).astype(np.float32)
        if img.max() > 1.5:
            img = img / 255.0
    else:
        try:
            from PIL import Image
        except ImportError as e:  # pragma: no cover
            raise RuntimeError("PIL is needed to decode image files (or pass .npy arrays)") from e
        img = np.asarray(Image.open(path).convert("RGB")).astype(np.float32) / 255.0
    t = torch.from_numpy(img).unsqueeze(0).permute(0, 3, 1, 2)
    t = F.interpolate(t, tuple(image_resolution), mode="bicubic", align_corners=True)
    return t.squeeze(0).permute(1, 2, 0).numpy()


class _ReadAhead:
    """Two staging slots and ONE background thread that reads files into host memory only (it never touches the GPU): while the
    caller copies a slot to the device, the thread fills the other one with the item expected next (the same step further).
    ``make_slot()`` -> a slot's buffers; ``read(idx, slot)`` fills them on the thread; ``prepare(idx, slot)`` runs before every
    read on the CALLER's thread (pinned allocations belong there).  A slot is refilled only after the H2D copies out of it have
    finished (the event ``release`` records)."""

    def __init__(self, n, make_slot, read, prepare=None, name="read-ahead"):
        from concurrent.futures import ThreadPoolExecutor
        self.n, self._read, self._prepare = n, read, prepare
        self._slots = [make_slot() for _ in range(2)]
        self._events = [None, None]
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix=name)
        self._pending = None   # (index, slot, future) of the read that is one ahead
        self._last = None      # the index asked for last: the next one is guessed from the step between the two
        self._slot = 0

    def _fill(self, idx, slot, ahead=False):
        if self._events[slot] is not None:
            self._events[slot].synchronize()
        if self._prepare is not None:
            self._prepare(idx, self._slots[slot])
        if ahead:
            return self._pool.submit(self._read, idx, self._slots[slot])
        self._read(idx, self._slots[slot])

    def acquire(self, idx):
        """-> the slot that holds item ``idx`` (read now unless it is the one read ahead)"""
        slot = 0
        if self._pending is not None:
            p_idx, p_slot, fut = self._pending
            self._pending = None
            fut.result()  # (a failed read raises here)
            slot = p_slot
            if p_idx != idx:  # a wrong guess: read into the other slot now
                slot = 1 - p_slot
                self._fill(idx, slot)
        else:
            self._fill(idx, slot)
        self._slot = slot
        return self._slots[slot]

    def release(self, idx):
        """the copies out of ``idx``'s slot are queued on the current stream: mark them, and read the next item into the other slot"""
        ev = torch.cuda.Event()
        ev.record()
        self._events[self._slot] = ev
        step = idx - self._last if self._last is not None and idx > self._last else 1
        self._last = idx
        if idx + step < self.n:
            other = 1 - self._slot
            self._pending = (idx + step, other, self._fill(idx + step, other, ahead=True))

    def close(self):
        self._pool.shutdown(wait=True)
        self._pending = None


# ------------------------------------------------------------------------------------------------------------------
# the general dataset's ground-truth files (general_dataset.py:75-158): what the host parses; the samples go to ops.gt_decode
GT_FORMATS = ("u4k", "eth3d", "mid", "cityscapes")
IMAGE_FORMATS = (None, "mid", "u4k", "cityscapes", "kitti")
KB_CROP = (352, 1216)  # general_dataset.py:45-50


def read_factor_file(path) -> float:
    """general_dataset.py:84-86: the depth factor is the first line of <val_factor>/<name>.txt"""
    with open(path, "r") as f:
        return float(f.readline())


def read_mid_calib(path):
    """general_dataset.py:117-123 -> (depth_factor = baseline x focal length, doffs): line 0 ``cam0=[f 0 cx; ...``, line 2 ``doffs=``,
    line 3 ``baseline=``, by the reference's own expressions"""
    with open(path, "r") as f:
        ext_l = f.readlines()
    cam_info_f = float(ext_l[0].strip().split(" ")[0].split("[")[1])
    base = float(ext_l[3].strip().split("=")[1])
    doffs = float(ext_l[2].strip().split("=")[1])
    return base * cam_info_f, doffs


def read_pfm_header(f):
    """datasets/utils.py:5-45 on an open binary file -> (width, height, little_endian, scale, payload offset).  ``Pf`` (one channel)
    only: the reference's own decoder cannot take edges of a colour map.  A malformed header raises ValueError."""
    import re
    header = f.readline().rstrip()
    if header == b"PF":
        raise ValueError("PFM: a colour map (PF) is no disparity map")
    if header != b"Pf":
        raise ValueError("Not a PFM file.")
    try:
        dim = re.match(r"^(\d+)\s(\d+)\s$", f.readline().decode("utf-8"))
    except UnicodeDecodeError:
        dim = None
    if not dim:
        raise ValueError("Malformed PFM header.")
    width, height = map(int, dim.groups())
    try:
        scale = float(f.readline().rstrip().decode("utf-8"))
    except (UnicodeDecodeError, ValueError):
        raise ValueError("Malformed PFM header.") from None
    if width < 1 or height < 1:
        raise ValueError("Malformed PFM header.")
    return width, height, scale < 0, abs(scale), f.tell()


def strip_image_name(name: str) -> str:
    """general_dataset.py:70-72"""
    return name.replace(".jpg", "").replace(".png", "").replace(".jpeg", "")


def strip_gt_name(name: str) -> str:
    """general_dataset.py:156-157"""
    return name.replace(".npy", "").replace(".exr", "")


def _png16_shape(path):
    """(h, w) of a 16-bit one-channel PNG from its IHDR"""
    with open(path, "rb") as f:
        head = f.read(26)
    if len(head) < 26 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise ValueError(f"{path}: not a PNG file")
    w, h, depth, ctype = struct.unpack(">IIBB", head[16:26])
    if depth != 16 or ctype != 0:
        raise ValueError(f"{path}: bit depth {depth}, colour type {ctype}; a Cityscapes disparity map is 16-bit greyscale")
    return h, w


def decode_image_u8(path, image_format, image_resolution):
    """the ``read_image`` branches that do not resize (general_dataset.py:23-25, :33-38, :39-53) up to the uint8 pixels ->
    (uint8 [h, w, 3], swap_rb): 'u4k' raw BGR bytes of ``image_resolution``; 'cityscapes' the RGB image; 'kitti' its kb-crop"""
    if image_format == "u4k":
        h, w = image_resolution
        if os.path.getsize(path) != h * w * 3:
            raise ValueError(f"{path}: {os.path.getsize(path)} bytes, expected {h * w * 3} ({h} x {w} x 3)")
        return np.fromfile(path, dtype=np.uint8).reshape(h, w, 3), True
    from PIL import Image
    image = Image.open(path).convert("RGB")
    if image_format == "kitti":
        if image.height < KB_CROP[0] or image.width < KB_CROP[1]:
            raise ValueError(f"{path}: {image.height} x {image.width} is smaller than the kb-crop {KB_CROP[0]} x {KB_CROP[1]}")
        top_margin, left_margin = int(image.height - KB_CROP[0]), int((image.width - KB_CROP[1]) / 2)
        image = image.crop((left_margin, top_margin, left_margin + KB_CROP[1], top_margin + KB_CROP[0]))
    return np.array(image), False  # (a writable copy: it becomes a tensor)


@DATASETS.register_module()
class ImageDataset:
    """general_dataset.py:161-245.  ``gt_format=None``: ground truth is metric depth as <gt_dir>/<basename>.npy.  ``gt_format`` in
    GT_FORMATS: the reference's DepthMap (:75-158) -- ``gt_files = sorted(listdir(gt_dir))`` paired with the images by position, the
    factor / calibration files found by its path replacements, the file's samples read into pinned staging buffers one item ahead
    (_ReadAhead) and decoded on the GPU: ops.disp_gt for 'u4k', ops.gt_decode for 'eth3d' / 'mid' / 'cityscapes' -> ``depth_gt``
    [1, 1, H, W] and ``boundary`` uint8 [H, W] on the device; ``get_metrics`` then scores with the resize inside the kernel.
    ``gt_shape`` replaces the reference's literal 4032 x 6048 (ETH3D's raw files carry no shape).  ``image_format`` selects
    read_image's branch (:22-62): None / 'mid' bicubic to ``image_resolution``; 'u4k' raw BGR bytes of ``image_resolution``;
    'cityscapes' RGB / 255 as it is; 'kitti' its 352 x 1216 kb-crop -- the last three through ops.u8_image."""
    ssi_metrics = False  # (the constructor's flag; an instance made without it scores as before)

    def __init__(self, rgb_image_dir, mode="", min_depth=1e-3, max_depth=80, gt_dir=None, image_resolution=(2160, 3840),
                 dataset_name="", network_process_size=(384, 512), resize_mode="zoe", edge_metrics=False, gt_format=None, image_format=None,
                 gt_shape=(4032, 6048), ssi_metrics=False):
        if gt_format == "gta":
            raise NotImplementedError("ImageDataset(gt_format='gta'): the .exr ground truth (general_dataset.py:96-101) needs imageio, "
                                      "which is not installed")
        if gt_format is not None and gt_format not in GT_FORMATS:
            raise ValueError(f"ImageDataset(gt_format={gt_format!r}): one of {', '.join(GT_FORMATS)} or None")
        if image_format not in IMAGE_FORMATS:
            raise ValueError(f"ImageDataset(image_format={image_format!r}): one of u4k, mid, cityscapes, kitti or None")
        self.rgb_image_dir = rgb_image_dir
        # edge_metrics: get_metrics adds the boundary metrics and the edge_* / noedge_* splits (metrics.compute_boundary_metrics)
        self.edge_metrics = bool(edge_metrics)
        # ssi_metrics: get_metrics adds the scale-and-shift-invariant scores (metrics.SSI_KEYS) over the plain pixel set
        self.ssi_metrics = bool(ssi_metrics)
        self.files = sorted(os.listdir(rgb_image_dir))
        # ground truth: metric depth as <gt_dir>/<basename>.npy, or (gt_format) the reference's per-dataset files
        self.gt_dir = gt_dir
        self.gt_format = gt_format if gt_dir is not None else None
        self.image_format = image_format
        self.gt_shape = (int(gt_shape[0]), int(gt_shape[1]))
        self._ahead = None
        self._meta = {}
        if self.gt_format is not None:
            self.gt_files = sorted(os.listdir(gt_dir))  # general_dataset.py:185: paired with the images by position
            if len(self.gt_files) != len(self.files):
                raise ValueError(f"ImageDataset: {len(self.files)} images in {rgb_image_dir} but {len(self.gt_files)} ground-truth files in "
                                 f"{gt_dir} (they are paired by their sorted position)")
        self.min_depth, self.max_depth = min_depth, max_depth
        self.dataset_name = dataset_name
        self.image_resolution = tuple(image_resolution)
        self.network_process_size = tuple(network_process_size)
        self.resize_mode = resize_mode

    def __len__(self):
        return len(self.files)

    def gt_meta(self, i) -> dict:
        """what the host parses of ground-truth file ``i`` (no sample is read): ``path``, ``shape`` (h, w), ``nbytes`` and ``offset`` of
        the samples in the file, and the decode arguments (``factor``, ``doffs``, ``byteswap``)"""
        if i in self._meta:
            return self._meta[i]
        import sys
        path = os.path.join(self.gt_dir, self.gt_files[i])
        m = dict(path=path, offset=0, factor=0.0, doffs=0.0, byteswap=False, item=4)
        if self.gt_format == "u4k":  # :82-89
            m["factor"] = read_factor_file(path.replace("val_gt", "val_factor").replace(".npy", ".txt"))
            m["shape"] = tuple(np.load(path, mmap_mode="r").shape)
            if len(m["shape"]) != 2:
                raise ValueError(f"{path}: disparity of shape {m['shape']}, expected [H, W]")
        elif self.gt_format == "eth3d":  # :104-106 (the shape is a literal there)
            m["shape"] = self.gt_shape
            if os.path.getsize(path) != self.gt_shape[0] * self.gt_shape[1] * 4:
                raise ValueError(f"{path}: {os.path.getsize(path)} bytes, expected {self.gt_shape[0]} x {self.gt_shape[1]} float32 (gt_shape)")
        elif self.gt_format == "mid":  # :115-125
            m["factor"], m["doffs"] = read_mid_calib(path.replace("gts", "calibs").replace(".pfm", ".txt"))
            with open(path, "rb") as f:
                try:
                    w, h, little, _scale, m["offset"] = read_pfm_header(f)
                except ValueError as e:
                    raise ValueError(f"{path}: {e}") from None
            m["shape"], m["byteswap"] = (h, w), little != (sys.byteorder == "little")
            if os.path.getsize(path) - m["offset"] != h * w * 4:
                raise ValueError(f"{path}: {os.path.getsize(path) - m['offset']} payload bytes, expected {h} x {w} float32")
        else:  # cityscapes :142
            m["shape"], m["item"] = _png16_shape(path), 2
        m["nbytes"] = m["shape"][0] * m["shape"][1] * m["item"]
        self._meta[i] = m
        return m

    def _prepare(self, i, slot):
        """(caller's thread) the slot's pinned buffer holds file ``i``'s samples"""
        need = self.gt_meta(i)["nbytes"]
        if slot["buf"] is None or slot["buf"].numel() < need:
            slot["buf"] = torch.empty((need,), dtype=torch.uint8).pin_memory()

    def _read(self, i, slot):
        """(background thread: files and host memory only) the samples of ground-truth file ``i`` as the file holds them, and the
        image's pixels when its branch needs no resize"""
        m = self.gt_meta(i)
        view = slot["buf"].numpy()[:m["nbytes"]]
        if self.gt_format == "u4k":
            np.copyto(view.view(np.float32).reshape(m["shape"]), np.load(m["path"], mmap_mode="r"), casting="unsafe")  # .astype(float32)
        elif self.gt_format == "cityscapes":
            from PIL import Image
            a = np.asarray(Image.open(m["path"]))  # cv2.imread(path, IMREAD_UNCHANGED) of a 16-bit PNG: its uint16 samples
            if a.shape != m["shape"] or a.dtype.itemsize != 2:
                raise ValueError(f"{m['path']}: decoded to {a.dtype} {a.shape}, expected uint16 {m['shape']}")
            np.copyto(view.view(np.uint16).reshape(m["shape"]), a, casting="unsafe")
        else:
            with open(m["path"], "rb") as f:
                f.seek(m["offset"])
                if f.readinto(memoryview(view)) != m["nbytes"]:
                    raise ValueError(f"{m['path']}: short read")
        slot["image"] = None
        if self.image_format in ("u4k", "cityscapes", "kitti"):
            slot["image"] = decode_image_u8(os.path.join(self.rgb_image_dir, self.files[i]), self.image_format, self.image_resolution)

    def close(self):
        if self._ahead is not None:
            self._ahead.close()
            self._ahead = None

    def _image(self, name, decoded=None):
        from . import ops
        path = os.path.join(self.rgb_image_dir, name)
        if self.image_format in (None, "mid"):
            # image_hr is resized on the device (prv2_bicubic_resize); image_lr is produced there too by model.resizer
            return read_image_device(path, self.image_resolution)
        pixels, swap = decoded if decoded is not None else decode_image_u8(path, self.image_format, self.image_resolution)
        return ops.u8_image(torch.from_numpy(np.ascontiguousarray(pixels)).cuda(), swap_rb=swap)

    def _getitem_gt(self, i):
        """an item with the reference's ground truth: the samples from the staging slot to the device, decoded there"""
        from . import ops
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(i)
        if self._ahead is None:
            self._ahead = _ReadAhead(len(self), lambda: dict(buf=None, image=None), self._read, self._prepare, name="gt-read")
        slot = self._ahead.acquire(i)
        m = self.gt_meta(i)
        raw = slot["buf"][:m["nbytes"]].cuda(non_blocking=True)
        decoded = slot["image"]
        self._ahead.release(i)
        if self.gt_format == "cityscapes":
            depth, boundary = ops.gt_decode(raw.view(torch.uint16).reshape(m["shape"]), "cityscapes", th=1.0)
        else:
            src = raw.view(torch.float32).reshape(m["shape"])
            if self.gt_format == "u4k":
                depth, boundary = ops.disp_gt(src, m["factor"], 1.0)
            elif self.gt_format == "eth3d":
                depth, boundary = ops.gt_decode(src, "eth3d", th=1.0)
            else:  # the PFM payload as the file holds it: bottom-to-top rows, its own byte order
                depth, boundary = ops.gt_decode(src, "mid", factor=m["factor"], doffs=m["doffs"], th=1.0, flip=True, byteswap=m["byteswap"])
        name = self.files[i]
        return dict(image_hr=self._image(name, decoded), img_file_basename=strip_image_name(name), depth_gt=depth[None, None],
                    boundary=boundary)

    def __getitem__(self, i):
        if self.gt_format is not None:
            return self._getitem_gt(i)
        name = self.files[i]
        item = dict(image_hr=self._image(name), img_file_basename=os.path.splitext(name)[0])
        if self.gt_dir is not None:
            from .metrics import get_boundaries
            gt = np.load(os.path.join(self.gt_dir, item["img_file_basename"] + ".npy")).astype(np.float32)
            item["depth_gt"] = torch.from_numpy(gt)[None, None]
            item["boundary"] = torch.from_numpy(get_boundaries(gt, th=1, dilation=0))
        return item

    def get_metrics(self, depth_gt, result, disp_gt_edges=None, **kw):
        """general_dataset.py:236-245 (a GPU ``result`` is scored where it is: metrics.compute_metrics_device).  With
        ``edge_metrics`` also the boundary metrics (cityscapes_dataset.py:340-403; GT edges = extract_edges(gt, 'log'), no
        segmentation map) and the edge_* / noedge_* splits of every metric (scannet_dataset.py:221-243)."""
        from .metrics import compute_metrics, compute_metrics_device, compute_metrics_fused
        dev = isinstance(result, torch.Tensor) and result.is_cuda
        score = compute_metrics_device if dev else compute_metrics
        if self.gt_format is not None:  # the ground truth is on the device: one fused pass, the prediction sampled inside it
            def score(gt, pred, **kw):
                return compute_metrics_fused(gt, pred, fuse_resize=True, **kw)
        common = dict(disp_gt_edges=disp_gt_edges, min_depth_eval=self.min_depth, max_depth_eval=self.max_depth, garg_crop=False,
                      eigen_crop=False, dataset=self.dataset_name)
        out = score(depth_gt, result, **common)
        if self.edge_metrics:
            out.update(self._edge_metrics(depth_gt, result, dev, score, common))
        if self.ssi_metrics:  # (losses.py:523-544, :600-700) on the device whenever the maps are there, else the host restatement
            from .metrics import compute_ssi_metrics, compute_ssi_metrics_fused
            common.pop("disp_gt_edges")
            if self.gt_format is not None or dev:
                out.update(compute_ssi_metrics_fused(depth_gt, result, fuse_resize=True, **common))
            else:
                out.update(compute_ssi_metrics(depth_gt, result, **common))
        return out

    def _edge_metrics(self, depth_gt, result, dev, score, common):
        """boundary metrics of the prediction (bilinearly resized to the GT's shape) against the GT's log-depth Canny edges at the
        valid pixels, then every depth metric inside / outside the 7 x 7-widened GT edges; on the device when ``result`` is there"""
        from . import metrics as M
        gt = torch.as_tensor(depth_gt)
        pred = result if result.dim() == 4 else result.reshape(1, 1, *result.shape[-2:])
        if pred.shape[-2:] != gt.shape[-2:]:
            pred = F.interpolate(pred, gt.shape[-2:], mode="bilinear", align_corners=False)
        if dev:
            g = gt.to(result.device).float().squeeze()
            ge, pe = M.extract_edges_device(g, "log"), M.extract_edges_device(pred.float(), "log")
            out = M.compute_boundary_metrics_device(ge, pe, (g > self.min_depth) & (g < self.max_depth))
            from . import ops
            region = ops.binary_dilate(ge, 7)[0]
        else:
            g = gt.float().squeeze().numpy()
            ge, pe = M.extract_edges(g, "log"), M.extract_edges(pred, "log")
            out = M.compute_boundary_metrics(ge, pe, (g > self.min_depth) & (g < self.max_depth))
            region = torch.from_numpy(M.binary_dilate(ge, 7))
        for name, mask in (("edge", region), ("noedge", ~region)):
            out.update({f"{name}_{k}": v for k, v in score(depth_gt, result, additional_mask=mask, **common).items()})
        return out


@DATASETS.register_module()
class UnrealStereo4kDataset:
    """estimator/datasets/u4k_dataset.py:20-233, inference mode: the frames of a split file with their ground truth, decoded on the
    GPU.  Per item the host only reads the two files (``<image>.raw``: BGR bytes; ``Disp0/*.npy``: disparity) into pinned staging
    buffers and copies them to the device; ops.u8_image makes ``image_hr`` (RGB / 255, CHW, bit-equal to the reference's numpy
    expression) and ops.disp_gt makes ``depth_gt`` = depth_factor / disparity and ``boundary`` = get_boundaries(disparity, th=1) in
    one pass.  The files of the NEXT index are read one item ahead on a single background thread (files and host memory only: it
    never touches the GPU).  ``get_metrics`` is metrics.compute_metrics_fused.  ``image_raw_shape`` replaces the reshape the
    reference hard-codes to (2160, 3840).  Not built: ``mode='train'`` (augmentation, crops) and ``consistency=True``."""

    dataset_name = "u4k"
    ssi_metrics = False  # (the constructor's flag)

    def __init__(self, mode, data_root, split, transform_cfg, min_depth, max_depth, consistency=False, overlap=0, patch_raw_shape=(540, 960),
                 resize_mode="zoe", pre_norm_bbox=True, image_raw_shape=(2160, 3840), ssi_metrics=False):
        if mode == "train":
            raise NotImplementedError("UnrealStereo4kDataset(mode='train'): the training pipeline (aug_rotate / aug_color / aug_flip / "
                                      "random_crop, u4k_dataset.py:131-213) is not built; inference modes only")
        if consistency:
            raise NotImplementedError("UnrealStereo4kDataset(consistency=True): the consistency crops (u4k_dataset.py:159-184) are not "
                                      "built; Tester.run_consistency makes its crops itself")
        if resize_mode not in ("zoe", "depth-anything"):
            raise NotImplementedError(f"UnrealStereo4kDataset(resize_mode={resize_mode!r})")  # u4k_dataset.py:48-55
        self.mode, self.data_root, self.split = mode, data_root, split
        self.min_depth, self.max_depth = min_depth, max_depth
        self.transform_cfg = transform_cfg
        self.network_process_size = tuple(transform_cfg["network_process_size"])
        self.resize_mode = resize_mode
        self.image_raw_shape = (int(image_raw_shape[0]), int(image_raw_shape[1]))
        self.ssi_metrics = bool(ssi_metrics)  # get_metrics adds the scale-and-shift-invariant scores (metrics.SSI_KEYS)
        self.data_infos = self.load_data_list()
        self._ahead = None     # the staging slots and their reader (_ReadAhead), made by the first item

    def load_data_list(self):
        """u4k_dataset.py:68-117: 'img_l img_r disp_l disp_r' per line; the image's suffix becomes ``raw``; focal length and baseline
        from the Extrinsics0 / Extrinsics1 text files beside the disparity; sorted by image path"""
        if self.split is None:
            raise NotImplementedError("UnrealStereo4kDataset needs a split file (u4k_dataset.py:113-114)")
        infos = []
        with open(self.split) as f:
            for line in f:
                if not line.strip():
                    continue
                img_l, _img_r, disp_l, _disp_r = line.strip().split(" ")
                img_l = img_l[:-3] + "raw"
                info = dict(depth_map_path=os.path.join(self.data_root, disp_l), img_path=os.path.join(self.data_root, img_l), filename=img_l)
                ext = []
                for cam in ("Extrinsics0", "Extrinsics1"):
                    with open(info["depth_map_path"].replace("Disp0", cam).replace("npy", "txt")) as fe:
                        ext.append(fe.readlines())
                info["focal"] = float(ext[0][0].split(" ")[0])
                info["depth_factor"] = abs(float(ext[0][1].split(" ")[3]) - float(ext[1][1].split(" ")[3])) * info["focal"]
                info["img_file_basename"] = os.path.splitext(img_l)[0].replace("/", "_")[1:]  # u4k_dataset.py:155-156
                infos.append(info)
        return sorted(infos, key=lambda x: x["img_path"])

    def __len__(self):
        return len(self.data_infos)

    def _read(self, idx, slot):
        """the two files of frame ``idx`` into staging slot ``slot`` (runs on the background thread: host memory only)"""
        img, disp = slot
        info = self.data_infos[idx]
        view = img.numpy().reshape(-1)
        with open(info["img_path"], "rb") as f:
            n = f.readinto(memoryview(view))
        if n != view.size or os.path.getsize(info["img_path"]) != view.size:
            raise ValueError(f"{info['img_path']}: {os.path.getsize(info['img_path'])} bytes, expected {view.size} "
                             f"({self.image_raw_shape[0]} x {self.image_raw_shape[1]} x 3)")
        d = np.load(info["depth_map_path"], mmap_mode="r")
        if d.shape != self.image_raw_shape:
            raise ValueError(f"{info['depth_map_path']}: disparity {d.shape}, expected {self.image_raw_shape}")
        np.copyto(disp.numpy(), d, casting="unsafe")  # == .astype(np.float32)

    def _make_slot(self):
        h, w = self.image_raw_shape
        return (torch.empty((h, w, 3), dtype=torch.uint8).pin_memory(), torch.empty((h, w), dtype=torch.float32).pin_memory())

    def close(self):
        if self._ahead is not None:
            self._ahead.close()
            self._ahead = None

    def __getitem__(self, idx):
        from . import ops
        idx = int(idx)
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        if self._ahead is None:
            self._ahead = _ReadAhead(len(self), self._make_slot, self._read, name="u4k-read")
        img, disp = self._ahead.acquire(idx)
        raw = img.cuda(non_blocking=True)
        d = disp.cuda(non_blocking=True)
        self._ahead.release(idx)  # (the next index, the same step further, is read into the other slot meanwhile)
        info = self.data_infos[idx]
        depth, boundary = ops.disp_gt(d, info["depth_factor"], 1.0)
        return dict(image_hr=ops.u8_image(raw, swap_rb=True), depth_gt=depth[None, None], boundary=boundary,
                    img_file_basename=info["img_file_basename"])

    def get_metrics(self, depth_gt, result, disp_gt_edges=None, **kw):
        """u4k_dataset.py:232-233 through the fused kernel (a host ``result`` is copied to the device first)"""
        from .metrics import compute_metrics_fused, compute_ssi_metrics_fused
        common = dict(min_depth_eval=self.min_depth, max_depth_eval=self.max_depth, garg_crop=False, eigen_crop=False, dataset="")
        out = compute_metrics_fused(depth_gt, result, disp_gt_edges=disp_gt_edges, **common)
        if self.ssi_metrics:
            out.update(compute_ssi_metrics_fused(depth_gt, result, **common))
        return out


ETH_METRIC_KEYS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel", "see")  # compute_metrics' order


def eth_metric_order(fused: dict) -> dict:
    """compute_metrics_fused(region=...)'s dict in the reference's order (eth_dataset.py:277-289, :304-335): ``edge_*``, ``noedge_*``, then
    the plain keys"""
    plain = [k for k in fused if not k.startswith(("edge_", "noedge_"))]
    return {pre + k: fused[pre + k] for pre in ("edge_", "noedge_", "") for k in plain}


@DATASETS.register_module()
class ETHDataset:
    """estimator/datasets/eth_dataset.py:23-385, inference modes: the photographs of a split file with their raw float32 ground truth.
    One background thread (_ReadAhead: files and host memory only) decodes the NEXT image with PIL (``convert("RGB")``) and reads the
    raw floats, both into pinned buffers; on the device ops.u8_image_resize makes ``image_hr`` (bytes / 255, bilinear
    align_corners=True to ``transform_cfg.input_size_shallow`` -- only the bytes cross PCIe; without that key ops.u8_image) and
    ops.gt_decode('eth3d') makes ``depth_gt`` [1, 1, H, W] (non-finite -> 0) and ``boundary``.  ``get_metrics`` finds the reference's
    edge area from the IMAGE gradient on the GPU (ops.image_edge_region) and scores inside it, outside it and everywhere in one fused
    pass.  ``gt_shape`` replaces the reference's literal 4032 x 6048 (the raw files carry no shape).  ``overlap``, ``crop_strategy`` and
    ``stitcher_stage`` are accepted and stored, but the crops of an item (``crops_image_hr`` / ``crop_depths`` / ``bboxs``, :194-221) are
    not built: Tester.run_consistency makes its own crops.  Not built: ``mode='train'`` and ``transform_cfg.random_crop``."""

    dataset_name = "eth3d"
    ssi_metrics = False  # (the constructor's flag)

    def __init__(self, mode, split, transform_cfg, min_depth, max_depth, stitcher_stage=0, overlap=0, crop_strategy="random",
                 resize_mode="zoe", gt_shape=(4032, 6048), ssi_metrics=False):
        if mode == "train":
            raise NotImplementedError("ETHDataset(mode='train'): the training pipeline (aug_rotate / aug_color / aug_flip, "
                                      "eth_dataset.py:144-167) is not built; inference modes only")
        if transform_cfg.get("random_crop", False):
            raise NotImplementedError("ETHDataset(transform_cfg.random_crop): the random crops (eth_dataset.py:179-190) are not built")
        if resize_mode not in ("zoe", "depth-anything"):
            raise NotImplementedError(f"ETHDataset(resize_mode={resize_mode!r})")  # eth_dataset.py:49-56
        self.mode, self.split = mode, split
        self.min_depth, self.max_depth = min_depth, max_depth
        self.transform_cfg = transform_cfg
        self.resize_mode = resize_mode
        self.stitcher_stage, self.overlap, self.crop_strategy = stitcher_stage, overlap, crop_strategy
        self.gt_shape = (int(gt_shape[0]), int(gt_shape[1]))
        self.ssi_metrics = bool(ssi_metrics)  # get_metrics adds the scale-and-shift-invariant scores (metrics.SSI_KEYS), plain set only
        shallow = transform_cfg.get("input_size_shallow", None)
        self.input_size_shallow = None if shallow is None else (int(shallow[0]), int(shallow[1]))
        self.data_infos = self.load_data_list()
        self._ahead = None

    def load_data_list(self):
        """eth_dataset.py:96-126: 'img depth' per line (absolute paths), sorted by image path; the basename of :238-239"""
        if self.split is None:
            raise NotImplementedError("ETHDataset needs a split file (eth_dataset.py:121-122)")
        infos = []
        with open(self.split) as f:
            for line in f:
                if not line.strip():
                    continue
                img, depth_map = line.strip().split(" ")
                infos.append(dict(img_path=img, depth_map_path=depth_map,
                                  img_file_basename=os.path.splitext(img)[0].replace("/", "_")[1:]))
        return sorted(infos, key=lambda x: x["img_path"])

    def __len__(self):
        return len(self.data_infos)

    def check_gt_file(self, idx):
        """the raw ground truth of item ``idx`` holds gt_shape float32 values, or ValueError naming the file -> its path"""
        path = self.data_infos[idx]["depth_map_path"]
        h, w = self.gt_shape
        if os.path.getsize(path) != h * w * 4:
            raise ValueError(f"{path}: {os.path.getsize(path)} bytes, expected {h * w * 4} ({h} x {w} float32, gt_shape)")
        return path

    def _make_slot(self):
        return dict(img=None, gt=torch.empty(self.gt_shape, dtype=torch.float32).pin_memory(), shape=None)

    def _prepare(self, idx, slot):
        """(caller's thread) the slot's pinned image buffer holds item ``idx``'s pixels (PIL reads the header only here)"""
        from PIL import Image
        with Image.open(self.data_infos[idx]["img_path"]) as im:
            need = im.height * im.width * 3
        if slot["img"] is None or slot["img"].numel() < need:
            slot["img"] = torch.empty((need,), dtype=torch.uint8).pin_memory()

    def _read(self, idx, slot):
        """(background thread: files and host memory only) the decoded image and the raw floats of item ``idx``"""
        from PIL import Image
        info = self.data_infos[idx]
        a = np.asarray(Image.open(info["img_path"]).convert("RGB"))  # eth_dataset.py:133
        np.copyto(slot["img"].numpy()[:a.size].reshape(a.shape), a)
        slot["shape"] = a.shape[:2]
        path = self.check_gt_file(idx)
        view = slot["gt"].numpy().reshape(-1).view(np.uint8)
        with open(path, "rb") as f:
            if f.readinto(memoryview(view)) != view.size:
                raise ValueError(f"{path}: short read")

    def close(self):
        if self._ahead is not None:
            self._ahead.close()
            self._ahead = None

    def __getitem__(self, idx):
        from . import ops
        idx = int(idx)
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        if self._ahead is None:
            self._ahead = _ReadAhead(len(self), self._make_slot, self._read, self._prepare, name="eth-read")
        slot = self._ahead.acquire(idx)
        h, w = slot["shape"]
        raw = slot["img"][:h * w * 3].cuda(non_blocking=True).view(h, w, 3)
        gt = slot["gt"].cuda(non_blocking=True)
        self._ahead.release(idx)
        if self.input_size_shallow is not None:  # eth_dataset.py:158-161
            image = ops.u8_image_resize(raw, *self.input_size_shallow)
        else:
            image = ops.u8_image(raw, swap_rb=False)
        depth, boundary = ops.gt_decode(gt, "eth3d", th=1.0)  # :137-139 and get_boundaries(disp_gt, th=1, dilation=0), :235
        return dict(image_hr=image, depth_gt=depth[None, None], boundary=boundary, img_file_basename=self.data_infos[idx]["img_file_basename"])

    def get_metrics(self, depth_gt, result, disp_gt_edges=None, image_hr=None, **kw):
        """eth_dataset.py:259-290: the edge area from the image gradient (ops.image_edge_region), then the reference's three
        compute_metrics calls as ONE fused pass over the three pixel sets, the prediction's resize inside it -> ``edge_*``,
        ``noedge_*``, then the plain keys (the reference's order)"""
        from . import ops
        from .metrics import compute_metrics_fused, compute_ssi_metrics_fused
        if image_hr is None:
            raise ValueError("ETHDataset.get_metrics needs image_hr: its edge area comes from the image gradient (eth_dataset.py:261)")
        image = torch.as_tensor(image_hr).cuda().float()
        region = ops.image_edge_region(image.reshape(3, *image.shape[-2:]), *depth_gt.shape[-2:])  # ([1, 3, h, w] in the reference)
        common = dict(min_depth_eval=self.min_depth, max_depth_eval=self.max_depth, garg_crop=False, eigen_crop=False, dataset="", fuse_resize=True)
        out = eth_metric_order(compute_metrics_fused(depth_gt, result, disp_gt_edges=disp_gt_edges, region=region, **common))
        if self.ssi_metrics:  # after the reference's thirty keys, over the plain pixel set
            out.update(compute_ssi_metrics_fused(depth_gt, result, **common))
        return out

    def evaluate(self, results, **kw):
        """eth_dataset.py:292-385 without the table: np.nanmean of every key over the frames' metric dicts (a frame whose edge or
        no-edge set is empty has NaN there and does not poison the mean; a key that is NaN in every frame stays NaN)"""
        import warnings
        out = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", category=RuntimeWarning)  # "Mean of empty slice"
            for k in results[0]:
                out[k] = float(np.nanmean([float(r[k]) for r in results]))
        return out


def pseudo_label_uncertainty(uncertainty: np.ndarray, count_map: np.ndarray, n_tiles: int, count_thr: float):
    """-> (u, count) float64: ``uncertainty`` min-max normalised to [0, 1] (0 when it is flat), then 1 wherever fewer than
    ``count_thr * n_tiles`` tiles cover the pixel (tester.py:164-166, whose hard-coded 177 is the tile count of an r128 plan at patch_split_num 4 x 4)"""
    unc = uncertainty.astype(np.float64)
    lo, hi = float(unc.min()), float(unc.max())
    u = (unc - lo) / (hi - lo) if hi > lo else np.zeros_like(unc)
    count = count_map.astype(np.float64)
    u[count < count_thr * n_tiles] = 1.0
    return u, count


class RunnerInfo:
    def __init__(self, **kw):
        self.rank, self.save, self.gray_scale, self.work_dir = 0, False, False, "."
        self.__dict__.update(kw)


def collect_results(results, size):
    """mmengine.dist.collect_results_gpu as Tester.run uses it (estimator/tester/tester.py:124-127): the per-rank result lists
    of a frame-sharded run (frame f on rank f mod world) all-gathered as pickled objects and interleaved back into dataset
    order on rank 0 (the other ranks get None); a single process returns its own list."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return results
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, results)
    if dist.get_rank() != 0:
        return None
    ordered = []
    for i in range(max(len(p) for p in parts)):
        ordered.extend(p[i] for p in parts if i < len(p))
    return ordered[:size]


class Tester:
    """``Tester(config, runner_info, dataloader, model).run(cai_mode, process_num, image_raw_shape, patch_split_num)``"""

    def __init__(self, config, runner_info, dataloader, model):
        self.config, self.runner_info, self.dataloader, self.model = config, runner_info, dataloader, model

    @torch.no_grad()
    def run(self, cai_mode="m1", process_num=4, image_raw_shape=(2160, 3840), patch_split_num=(4, 4), seed=None, shard="frames",
            frame_batch=1):
        """``shard='frames'`` (the reference's data parallelism, tester.py:58: frame f on rank f mod world) or ``'patches'`` (every
        rank works on EVERY frame: its tiles are sharded over the ranks and gathered to rank 0, which blends, saves and scores --
        models._PatchModel.forward(shard=...)).  The loop knows its next frame: its low-resolution image is announced to the
        model, which runs that coarse forward beside the current frame's tiles (``next_image_lr``).
        ``frame_batch``: N frames per model call (the last group may be shorter; a frame-sharded run groups each rank's frames); the
        results are split per frame -- names, order, PNGs and metrics as with one frame per call, and bit-identical to it."""
        import random
        results = []
        rank, world = self.runner_info.rank, getattr(self.runner_info, "world_size", 1)
        patches = shard == "patches" and world > 1
        fb = max(1, int(frame_batch))
        if fb > 1 and patches:
            raise ValueError("frame_batch > 1 with shard='patches': the patch-sharded mode takes one frame per call")
        prefetch = bool(getattr(self.model, "needs_coarse", False))
        todo = list(range(len(self.dataloader))) if patches else list(range(rank, len(self.dataloader), world))
        groups = [todo[i:i + fb] for i in range(0, len(todo), fb)]
        stage = self.last_output_stage = self._output_stage()  # (kept: its bytes_d2h / files counters)

        def load(idxs):
            items = [self.dataloader[idx] for idx in idxs]
            hr = torch.stack([item["image_hr"] for item in items]).cuda()
            return items, hr, self.model.resizer(hr)

        nxt = load(groups[0]) if groups else None
        for n, idxs in enumerate(groups):
            items, hr, lr = nxt
            nxt = load(groups[n + 1]) if n + 1 < len(groups) else None
            kw = {}
            if seed is not None:
                if fb == 1:
                    random.seed(seed)
                else:  # (every frame's plan from the same seed, as one frame per call does)
                    kw["frame_seeds"] = [seed] * len(idxs)
            tile_cfg = dict(image_raw_shape=list(image_raw_shape), patch_split_num=list(patch_split_num))
            # with ground truth the frame is scored on the device (metrics.compute_metrics_device): ask for the device map
            if any(item.get("depth_gt") is not None for item in items) and getattr(self.model, "supports_return_device", False):
                kw.update(return_device=True)
            if stage is not None:  # the device output stage reads the maps where they are
                kw.update(return_device=True)
            if patches:
                kw.update(shard=(rank, world), gather_dst=0)
            if prefetch and nxt is not None:
                kw["next_image_lr"] = nxt[2]
            result, log = self.model(mode="infer", cai_mode=cai_mode, process_num=process_num, tile_cfg=tile_cfg,
                                     image_lr=lr, image_hr=hr, **kw)
            if result is None:  # patch-sharded: only rank 0 holds the map
                continue
            coarse = log.get("coarse_prediction")
            for f, item in enumerate(items):
                one = len(items) == 1
                self._emit(results, item, result if one else result[f:f + 1], coarse if one or coarse is None else coarse[f:f + 1],
                           image_raw_shape, stage)
        if stage is not None:
            stage.close()  # every file is on disk (or its error raised) before run returns
        if not patches:
            # collect results from all ranks (tester.py:124-127: collect_results_gpu); rank 0 evaluates the whole dataset
            allr = collect_results(results, len(self.dataloader))
            results = allr if allr is not None else results
        if results and "metrics" in results[0] and rank == 0:
            from .metrics import evaluate
            own = getattr(self.dataloader, "evaluate", None)  # a dataset's own aggregation (ETHDataset: nanmean)
            self.last_eval = (own or evaluate)([r["metrics"] for r in results])
        return results

    def _output_stage(self):
        """the run's ``output.OutputStage`` when ``runner_info.device_output`` and ``save`` are set (``output_workers`` threads,
        default 8; ``device_deflate``: zlib streams from the GPU too -- same pixels, other file bytes), else None.  The stage needs the maps on the device: a model without ``return_device`` is rejected."""
        deflate = bool(getattr(self.runner_info, "device_deflate", False))
        if deflate and not getattr(self.runner_info, "device_output", False):
            raise ValueError("device_deflate needs device_output (the zlib streams are made from the device route's scanlines)")
        if not (getattr(self.runner_info, "device_output", False) and self.runner_info.save):
            return None
        if not getattr(self.model, "supports_return_device", False):
            raise ValueError(f"device_output: {type(self.model).__name__} cannot return a device map (no return_device); use the host route")
        from .output import OutputStage
        return OutputStage(self.runner_info.work_dir, workers=getattr(self.runner_info, "output_workers", 8), device_deflate=deflate)

    def _emit_device(self, results, item, result, coarse, image_raw_shape, stage):
        """``_emit`` through the device output stage: the same files from scanlines produced on the GPU, the same result entry
        (its mean is a float64 sum on the device: equal to the host's float32 mean within that sum's rounding)"""
        if not result.is_cuda:
            raise ValueError("device_output: the model returned a host map")
        base = os.path.join(self.runner_info.work_dir, item["img_file_basename"])
        if getattr(self.runner_info, "gray_scale", False):
            cmap, pct = "gray_r", (2, 95)  # colorize's defaults, as _emit
        else:
            cmap, pct = ("magma_r" if getattr(self.dataloader, "dataset_name", "") == "cityscapes" else "Spectral"), (0, 100)
        stage.submit_frame(base, result, coarse, image_raw_shape, cmap=cmap, percentiles=pct)
        entry = dict(name=item["img_file_basename"], shape=tuple(result.shape), mean=float(result.mean(dtype=torch.float64)))
        if item.get("depth_gt") is not None:
            entry["metrics"] = self.dataloader.get_metrics(item["depth_gt"], result, disp_gt_edges=item.get("boundary"),
                                                           image_hr=item["image_hr"])
        results.append(entry)

    def _emit(self, results, item, result, coarse, image_raw_shape, stage=None):
        """one frame's outputs: PNGs (--save), its metrics and its result entry"""
        if stage is not None:
            return self._emit_device(results, item, result, coarse, image_raw_shape, stage)
        result_dev = result if result.is_cuda else None
        result = result.cpu()  # BaselinePretrain(target='coarse') hands back the device tensor (baseline_pretrain.py:464)
        if self.runner_info.save:
            os.makedirs(self.runner_info.work_dir, exist_ok=True)
            base = os.path.join(self.runner_info.work_dir, item["img_file_basename"])
            # raw depth as 16-bit PNG, multiplier 256 (tester.py:89-91)
            write_png16(base + "_uint16.png", (result.squeeze().numpy() * 256).astype("uint16"))
            from .metrics import colorize
            if getattr(self.runner_info, "gray_scale", False):
                color = colorize(result, cmap="gray_r")
            else:  # every dataset branch of tester.py:76-84 but cityscapes maps to Spectral, 0..100 percentiles
                cmap = "magma_r" if getattr(self.dataloader, "dataset_name", "") == "cityscapes" else "Spectral"
                color = colorize(result, cmap=cmap, vminp=0, vmaxp=100)
            write_png8(base + ".png", np.ascontiguousarray(color[:, :, :3]))
            from .metrics import depth_edges
            write_png8(base + "_edge.png", depth_edges(result).astype(np.uint8) * 255)  # tester.py:99-106
            if coarse is not None:  # absent for BaselinePretrain
                coarse_map = F.interpolate(coarse.cpu(), tuple(image_raw_shape), mode="bilinear")
                write_png8(base + "_coarse.png", np.ascontiguousarray(colorize(coarse_map, cmap="Spectral", vminp=0, vmaxp=100)[:, :, :3]))
        entry = dict(name=item["img_file_basename"], shape=tuple(result.shape), mean=float(result.mean()))
        if item.get("depth_gt") is not None:
            entry["metrics"] = self.dataloader.get_metrics(item["depth_gt"], result if result_dev is None else result_dev,
                                                           disp_gt_edges=item.get("boundary"), image_hr=item["image_hr"])
        results.append(entry)

    @torch.no_grad()
    def generate_pl(self, cai_mode="r32", process_num=4, image_raw_shape=(2160, 3840), patch_split_num=(4, 4), count_thr=0.05, seed=None,
                    frame_batch=1, uncert_metrics=False):
        """Pseudo labels for semi-supervised training (estimator/tester/tester.py:132-181): the model runs over the folder with
        ``return_uncertainty=True`` and, with ``runner_info.save``, writes per image under ``work_dir`` what the pseudo-label loader of
        the semi-supervised configs reads (estimator/datasets/cityscapes_dataset.py:115-123,202-214):
          <name>.png                colour depth (magma_r, gray_r with gray_scale; percentiles 0..100)
          <name>_uint16.png         depth x 256
          <name>_uncert_uint16.png  floor(u x 256), u = the uncertainty min-max normalised to [0, 1] and set to 1 where fewer than
                                    count_thr x (tiles of the frame's plan) tiles cover the pixel (0 everywhere when the map is flat)
          <name>_uncert.png         u coloured with jet, percentiles 0..100
          <name>_count_uint16.png   tile count x 256 (saturates at 65535: 256 tiles or more)
        Frames are dealt to the ranks as in ``run`` (frame f on rank f mod world) and grouped ``frame_batch`` per model call.
        Returns one dict per frame of this rank (name, shape, mean depth, tiles of the plan).
        ``uncert_metrics`` (tools/test.py --uncert-metrics; not in the reference): every frame whose item carries ``depth_gt`` is also
        scored on the device -- does the uncertainty mark the pixels where the depth is wrong? -- with the sparsification scores
        ``ause_abs_rel, aurg_abs_rel, ause_rmse, aurg_rmse`` (metrics.compute_uncertainty_metrics_fused on the model's ``uncertainty``
        and ``count_map`` with min_count = count_thr x tiles, inside the dataset's min_depth / max_depth) under the frame's key
        ``uncert_metrics``; ``self.last_eval`` becomes their per-key nanmean over the scored frames.  Items without ground truth are
        skipped; a result of another shape than the ground truth (an m-mode at the re-ensemble shape) is an error.  The files and
        the rest of the dicts do not change."""
        import random
        results = []
        rank, world = self.runner_info.rank, getattr(self.runner_info, "world_size", 1)
        fb = max(1, int(frame_batch))
        prefetch = bool(getattr(self.model, "needs_coarse", False))
        todo = list(range(rank, len(self.dataloader), world))
        groups = [todo[i:i + fb] for i in range(0, len(todo), fb)]
        device = getattr(self.model, "device", "cuda")
        stage = self.last_output_stage = self._output_stage()  # (kept: its bytes_d2h / files counters)

        def load(idxs):
            items = [self.dataloader[idx] for idx in idxs]
            hr = torch.stack([item["image_hr"] for item in items]).to(device)
            return items, hr, self.model.resizer(hr)

        nxt = load(groups[0]) if groups else None
        for n, idxs in enumerate(groups):
            items, hr, lr = nxt
            nxt = load(groups[n + 1]) if n + 1 < len(groups) else None
            kw = dict(return_uncertainty=True)
            if stage is not None:
                kw.update(return_device=True)
            score = bool(uncert_metrics) and any(item.get("depth_gt") is not None for item in items)
            if score and getattr(self.model, "supports_return_device", False):  # the maps stay where they are scored
                kw.update(return_device=True)
            if seed is not None:
                if len(idxs) == 1:
                    random.seed(seed)
                else:
                    kw["frame_seeds"] = [seed] * len(idxs)
            if prefetch and nxt is not None:
                kw["next_image_lr"] = nxt[2]
            tile_cfg = dict(image_raw_shape=list(image_raw_shape), patch_split_num=list(patch_split_num))
            result, log = self.model(mode="infer", cai_mode=cai_mode, process_num=process_num, tile_cfg=tile_cfg, image_lr=lr, image_hr=hr,
                                     **kw)
            # the plan's tile count (every frame of a call has the same passes; only random positions differ)
            n_tiles = sum(len(p["raw"]) for p in self.model.last_plan)
            for f, item in enumerate(items):
                scored = {}
                if score and item.get("depth_gt") is not None:
                    scored = dict(uncert_metrics=self._uncert_metrics(item, result[f:f + 1], log["uncertainty"][f:f + 1],
                                                                      log["count_map"][f:f + 1], count_thr * n_tiles, cai_mode))
                if stage is not None:  # the five files from scanlines produced on the GPU
                    depth = result[f:f + 1]
                    cmap = "gray_r" if getattr(self.runner_info, "gray_scale", False) else "magma_r"
                    stage.submit_pseudo_label(os.path.join(self.runner_info.work_dir, item["img_file_basename"]), depth,
                                              log["uncertainty"][f:f + 1], log["count_map"][f:f + 1], n_tiles, count_thr, cmap=cmap)
                    results.append(dict(name=item["img_file_basename"], shape=tuple(depth.shape),
                                        mean=float(depth.mean(dtype=torch.float64)), n_tiles=n_tiles, **scored))
                    continue
                depth = result[f:f + 1].cpu()
                entry = dict(name=item["img_file_basename"], shape=tuple(depth.shape), mean=float(depth.mean()), n_tiles=n_tiles, **scored)
                if self.runner_info.save:
                    self._write_pl(item["img_file_basename"], depth, log["uncertainty"][f:f + 1].cpu(), log["count_map"][f:f + 1].cpu(),
                                   n_tiles, count_thr)
                results.append(entry)
        if stage is not None:
            stage.close()
        if uncert_metrics:
            from .metrics import UNCERT_KEYS
            import warnings
            rows = [r["uncert_metrics"] for r in results if "uncert_metrics" in r]
            with warnings.catch_warnings():  # (a key that is NaN in every frame: its mean is NaN, silently)
                warnings.simplefilter("ignore", RuntimeWarning)
                self.last_eval = {k: float(np.nanmean([m[k] for m in rows])) for k in UNCERT_KEYS} if rows else {}
        return results

    def _uncert_metrics(self, item, depth, uncertainty, count_map, min_count, cai_mode):
        """one frame's sparsification scores (``generate_pl(uncert_metrics=True)``): maps [1, 1, H, W], on the device already when the
        model can return them there"""
        from .metrics import compute_uncertainty_metrics_fused
        gt = torch.as_tensor(item["depth_gt"])
        if tuple(depth.shape[-2:]) != tuple(gt.shape[-2:]):
            raise ValueError(f"uncert_metrics: {item['img_file_basename']}: the result of cai_mode {cai_mode!r} has shape "
                             f"{tuple(depth.shape[-2:])} but the ground truth {tuple(gt.shape[-2:])}; the maps are not resized -- r-modes "
                             "return the raw shape (m-modes the re-ensemble shape): use an r-mode with image_raw_shape = the ground truth's")
        dev = depth.device if depth.is_cuda else torch.device("cuda")
        h, w = gt.shape[-2:]
        g, d, u, c = (t.to(dev).float().reshape(h, w) for t in (gt, depth, uncertainty, count_map))
        return compute_uncertainty_metrics_fused(g, d, u, count=c, min_count=min_count, min_depth_eval=self.dataloader.min_depth,
                                                 max_depth_eval=self.dataloader.max_depth)

    def _write_pl(self, name, depth, uncertainty, count_map, n_tiles, count_thr):
        """one frame's pseudo-label files (``generate_pl``)"""
        from .metrics import colorize
        os.makedirs(self.runner_info.work_dir, exist_ok=True)
        base = os.path.join(self.runner_info.work_dir, name)
        cmap = "gray_r" if getattr(self.runner_info, "gray_scale", False) else "magma_r"
        write_png8(base + ".png", np.ascontiguousarray(colorize(depth, cmap=cmap, vminp=0, vmaxp=100)[:, :, :3]))
        write_png16(base + "_uint16.png", (depth.squeeze().numpy() * 256).astype("uint16"))
        u, count = pseudo_label_uncertainty(uncertainty.squeeze().numpy(), count_map.squeeze().numpy(), n_tiles, count_thr)
        write_png16(base + "_uncert_uint16.png", np.clip(np.floor(u * 256.0), 0, 65535).astype(np.uint16))
        write_png8(base + "_uncert.png", np.ascontiguousarray(colorize(u, cmap="jet", vminp=0, vmaxp=100)[:, :, :3]))
        write_png16(base + "_count_uint16.png", np.clip(count * 256.0, 0, 65535).astype(np.uint16))

    @torch.no_grad()
    def run_consistency(self, image_raw_shape=(2160, 3840), patch_split_num=(4, 4), overlap=270):
        """Seam-consistency protocol of the reference (estimator/tester/tester.py:211-321 with the U4K / ETH3D consistency
        crops, eth_dataset.py:86-93): the frame's sh x sw crops of patch_raw_shape are shifted towards the centre so that
        neighbours overlap by ``overlap`` pixels, each crop is predicted on its own (the reference drives ``mode='train'`` once
        per crop: coarse forward + that crop's ROI + refiner), resized bilinear(align_corners) to the crop's raw size, and the
        error is the mean |difference| over the strips two adjacent crops share (left and up neighbours, tester.py:250-293).
        Returns one dict per frame with ``consistency_error``; ``self.last_eval`` holds the dataset mean."""
        from . import ops
        sh, sw = patch_split_num
        H, W = image_raw_shape
        rh, rw = H // sh, W // sw
        half = overlap // 2

        def starts(n, size):  # eth_dataset.py:92-93 generalised: shift crop i by ((n - 1) - 2 i) * overlap / 2 towards the centre
            return [int(i * size + ((n - 1) - 2 * i) * overlap / 2) for i in range(n)]

        hs, ws = starts(sh, rh), starts(sw, rw)
        tiles = [(h, w) for h in hs for w in ws]
        tile_cfg = dict(image_raw_shape=list(image_raw_shape), patch_split_num=list(patch_split_num))
        results = []
        rank, world = self.runner_info.rank, getattr(self.runner_info, "world_size", 1)
        for idx in range(rank, len(self.dataloader), world):
            item = self.dataloader[idx]
            hr = item["image_hr"].unsqueeze(0).cuda()
            # the consistency dataset hands the model pre-normalised bboxs (pre_norm_bbox=True in every shipped config)
            pre = bool(getattr(getattr(self.model, "config", None), "get", lambda k, d: d)("pre_norm_bbox", True))
            preds = self.model.predict_tiles(self.model.resizer(hr), hr, tiles, tile_cfg, prenorm_bbox=pre)
            up = torch.empty((len(tiles), rh, rw, 1), device=preds.device)  # dense 1-channel NHWC == [K, rh, rw]
            ops.upsample_bilinear(ops.Feat(preds.view(len(tiles), preds.shape[-2], preds.shape[-1], 1)), rh, rw, out=ops.Feat(up))
            up = up.view(len(tiles), rh, rw)
            errs = []
            for ii in range(sh):
                for jj in range(sw):
                    cur = up[ii * sw + jj]
                    if jj > 0:  # left neighbour: its last ``overlap`` columns == my first ones
                        errs.append((up[ii * sw + jj - 1][:, -overlap:] - cur[:, :overlap]).abs().flatten())
                    if ii > 0:  # upper neighbour
                        errs.append((up[(ii - 1) * sw + jj][-overlap:, :] - cur[:overlap, :]).abs().flatten())
            ce = float(torch.cat(errs).mean()) if errs else 0.0
            entry = dict(name=item["img_file_basename"], consistency_error=ce)
            self.last_crops = up  # [sh * sw, rh, rw] on the device (tests compare them with the reference's)
            if self.runner_info.save:  # the stitched centres (tester.py:243-247) as a colour map
                os.makedirs(self.runner_info.work_dir, exist_ok=True)
                full = torch.zeros((H, W))
                for k, (h, w) in enumerate(tiles):
                    full[h + half:h + rh - half, w + half:w + rw - half] = up[k][half:rh - half, half:rw - half].cpu()
                from .metrics import colorize
                write_png8(os.path.join(self.runner_info.work_dir, entry["name"] + ".png"), np.ascontiguousarray(colorize(full[None, None])[:, :, :3]))
            results.append(entry)
        self.last_eval = dict(consistency_error=float(np.mean([r["consistency_error"] for r in results]))) if results else {}
        return results

    @torch.no_grad()
    def benchmark(self, cai_mode="m1", process_num=4, image_raw_shape=(2160, 3840), patch_split_num=(4, 4), repeat_times=10,
                  log_interval=10, num_warmup=20, total_iters=50, seed=None):
        """The reference's own throughput protocol (estimator/tester/tester.py:325-406): ``repeat_times`` passes over the
        dataloader, each timing frames ``num_warmup`` .. ``total_iters`` one by one (synchronize, perf_counter, model(...),
        synchronize), fps = frames / summed time; reports the mean and variance over the passes plus the model's FLOPs and
        parameter count (mmengine's get_model_complexity_info there; here the per-launch algorithmic 2*MAC accounting of
        ops.PROFILER and the state-dict spec) and writes ``<work_dir>/benchmark.txt``.  The dataset is cycled when it holds
        fewer than ``total_iters`` frames (the reference simply stops early and divides by zero)."""
        import random
        import time
        from . import ops
        n = len(self.dataloader)
        if n == 0:
            raise ValueError("benchmark: empty dataset")
        tile_cfg = dict(image_raw_shape=list(image_raw_shape), patch_split_num=list(patch_split_num))
        items = {}

        def frame(i):
            if i % n not in items:  # decode + device resize once per file: the reference times model(...) only
                hr = self.dataloader[i % n]["image_hr"].unsqueeze(0).cuda()
                items[i % n] = (hr, self.model.resizer(hr))
            return items[i % n]

        bench = dict(unit="img / s")
        fps_list = []
        for rep in range(repeat_times):
            pure = 0.0
            for i in range(total_iters):
                hr, lr = frame(i)
                if seed is not None:
                    random.seed(seed)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                self.model(mode="infer", cai_mode=cai_mode, process_num=process_num, tile_cfg=tile_cfg, image_lr=lr, image_hr=hr)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if i >= num_warmup:
                    pure += dt
                    if (i + 1) % log_interval == 0 and self.runner_info.rank == 0:
                        print(f"Done image [{i + 1:<3}/ {total_iters}], fps: {(i + 1 - num_warmup) / pure:.3f} img / s")
            fps = (total_iters - num_warmup) / pure
            bench[f"overall_fps_{rep + 1}"] = round(fps, 2)
            fps_list.append(fps)
        bench["average_fps"] = round(float(np.mean(fps_list)), 2)
        bench["fps_variance"] = round(float(np.var(fps_list)), 4)
        hr, lr = frame(0)
        ops.PROFILER.start()
        self.model(mode="infer", cai_mode=cai_mode, process_num=process_num, tile_cfg=tile_cfg, image_lr=lr, image_hr=hr)
        torch.cuda.synchronize()
        ops.PROFILER.stop()
        summ = ops.PROFILER.summary()
        bench["flops"] = float(sum(d["flops"] for d in summ.values()))
        bench["params"] = int(sum(int(np.prod(shp)) for shp in self.model.spec().values()))
        if self.runner_info.rank == 0:
            os.makedirs(self.runner_info.work_dir, exist_ok=True)
            with open(os.path.join(self.runner_info.work_dir, "benchmark.txt"), "w") as f:
                f.write("kernel, launches, GFLOP (2*MAC) per frame\n")
                for tag, d in sorted(summ.items(), key=lambda kv: -kv[1]["flops"]):
                    f.write(f"{tag}, {d['launches']}, {d['flops'] / 1e9:.1f}\n")
                f.write(f"\nModel Flops: {bench['flops'] / 1e12:.3f} T per frame\nModel Parameters: {bench['params'] / 1e6:.1f} M\n")
                f.write(f"\n\n Average fps of {repeat_times} evaluations: {bench['average_fps']}")
                f.write(f"\n\n The variance of {repeat_times} evaluations: {bench['fps_variance']}\n")
        return bench
