"""The datasets of the tester: what an item is made of, and how it is scored.

ImageDataset        estimator/datasets/general_dataset.py:64-245 (folder of images -> image_hr / image_lr; with ``gt_format`` the
                    ground truth of a u4k / eth3d / mid / cityscapes folder, decoded on the GPU -> depth_gt / boundary)
UnrealStereo4kDataset  estimator/datasets/u4k_dataset.py:20-233 (split file -> image_hr / depth_gt / boundary, decoded on the GPU)
ETHDataset          estimator/datasets/eth_dataset.py:23-385 (split file -> image_hr resized on the GPU / depth_gt / boundary; every
                    metric also inside and outside the image's edge area, found on the GPU)
CityScapesDataset   estimator/datasets/cityscapes_dataset.py:27-501 (split file -> image_hr / depth_gt / boundary / seg_image, decoded on
                    the GPU with the file's own camera; depth metrics away from class boundaries and image edges, boundary metrics
                    on segmentation edges that are ground-truth depth edges)
KittiDataset        estimator/datasets/kitti_dataset.py:22-295 (split file -> image_hr / depth_gt / boundary: the 16-bit depth PNG read through
                    the 352 x 1216 kb-crop window on the GPU, / 256; the ten metrics inside the Garg crop)
ScanNetDataset      estimator/datasets/scannet_dataset.py:25-404 (split file -> image_hr / depth_gt / boundary: the 16-bit depth PNG brought
                    to the image's size by Pillow's NEAREST rule on the GPU, / 1000; every metric also inside and outside the widened
                    ground-truth depth edges)
``ssi_metrics=True`` (tools/test.py --ssi-metrics) on any of the datasets: get_metrics adds the scale-and-shift-invariant scores
                    of estimator/models/losses.py:523-544, :600-700 (metrics.SSI_KEYS; two fused GPU passes, csrc/ssi_eval.hip)
``boundary_f1=True`` (tools/test.py --boundary-f1) on any of the datasets: get_metrics adds the scale-invariant boundary F1 of Depth Pro
                    (metrics.BOUNDARY_KEYS; one fused GPU pass, csrc/boundary_eval.hip) after every other key
read_image          estimator/datasets/general_dataset.py:22-62 (RGB/255 -> bicubic, align_corners=True)
_ReadAhead / _StagedDataset  the two staging slots and the one background reader that the datasets share
Not built: the ``gta`` ground truth (general_dataset.py:96-101: .exr files need imageio, which is absent).  CityScapesDataset, KittiDataset
and ScanNetDataset are classes here but no registry entries (see there).  Without ``gt_format`` ground truth is metric depth as <basename>.npy files.
"""
from __future__ import annotations

import os
import struct

import numpy as np
import torch
import torch.nn.functional as F

from .registry import DATASETS


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


def _read_exact(path, view, offset=0):
    """the file's bytes from ``offset`` on fill the uint8 array ``view``"""
    with open(path, "rb") as f:
        f.seek(offset)
        if f.readinto(memoryview(view)) != view.size:
            raise ValueError(f"{path}: short read")


class _StagedDataset:
    """What the datasets share: the read-ahead's life cycle and the two ends of ``get_metrics`` (``_common``, ``_with_extras``).
    A subclass gives ``_make_slot()``, ``_read(idx, slot)`` and, if it needs one, ``_prepare(idx, slot)`` (_ReadAhead's three
    callbacks); its ``__getitem__`` queues its own copies out of the slot between ``_acquire`` and ``_release``."""
    ssi_metrics = False  # (the constructor's flag; an instance made without it scores as before)
    boundary_f1 = False  # (likewise)
    _ahead = None        # the staging slots and their reader, made by the first item
    _prepare = None
    _reader_name = "read-ahead"

    def _acquire(self, idx):
        """-> (int(idx), the staging slot that holds item ``idx``)"""
        idx = int(idx)
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        if self._ahead is None:
            self._ahead = _ReadAhead(len(self), self._make_slot, self._read, self._prepare, name=self._reader_name)
        return idx, self._ahead.acquire(idx)

    def _release(self, idx):
        """the copies out of ``idx``'s slot are queued (the next index, the same step further, is read into the other slot meanwhile)"""
        self._ahead.release(idx)

    def close(self):
        if self._ahead is not None:
            self._ahead.close()
            self._ahead = None

    def _common(self, dataset="", **extra):
        """compute_metrics' arguments that no dataset varies (``extra``: fuse_resize)"""
        return dict(min_depth_eval=self.min_depth, max_depth_eval=self.max_depth, garg_crop=False, eigen_crop=False, dataset=dataset, **extra)

    def _with_extras(self, out, ssi, depth_gt, result, common):
        """``out``, and after its keys the opt-in scores of the plain pixel set: with ``ssi_metrics`` (losses.py:523-544, :600-700)
        ``ssi``'s scores, then with ``boundary_f1`` the scale-invariant boundary F1 (metrics.BOUNDARY_KEYS) -- by the fused route
        wherever ``ssi`` is the fused one (with its ``fuse_resize``), by the host specification otherwise"""
        if self.ssi_metrics:
            out.update(ssi(depth_gt, result, **common))
        if self.boundary_f1:
            from functools import partial
            from . import metrics as M
            fused = partial(M.compute_boundary_f1_fused, **getattr(ssi, "keywords", {}))  # (ImageDataset hands a partial with fuse_resize)
            out.update((M.compute_boundary_f1 if ssi is M.compute_ssi_metrics else fused)(depth_gt, result, **common))
        return out

    def boundary_args(self):
        """compute_metrics' arguments the dataset's boundary F1 is scored with (KittiDataset: inside its Garg crop) -- what the tester
        scores the coarse prediction with, next to the result's"""
        return self._common(getattr(self, "dataset_name", ""))


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


def _png16_shape(path, what="a Cityscapes disparity map"):
    """(h, w) of a 16-bit one-channel PNG from its IHDR (``what``: the kind of file the message names)"""
    with open(path, "rb") as f:
        head = f.read(26)
    if len(head) < 26 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise ValueError(f"{path}: not a PNG file")
    w, h, depth, ctype = struct.unpack(">IIBB", head[16:26])
    if depth != 16 or ctype != 0:
        raise ValueError(f"{path}: bit depth {depth}, colour type {ctype}; {what} is 16-bit greyscale")
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
class ImageDataset(_StagedDataset):
    """general_dataset.py:161-245.  ``gt_format=None``: ground truth is metric depth as <gt_dir>/<basename>.npy.  ``gt_format`` in
    GT_FORMATS: the reference's DepthMap (:75-158) -- ``gt_files = sorted(listdir(gt_dir))`` paired with the images by position, the
    factor / calibration files found by its path replacements, the file's samples read into pinned staging buffers one item ahead
    (_ReadAhead) and decoded on the GPU: ops.disp_gt for 'u4k', ops.gt_decode for 'eth3d' / 'mid' / 'cityscapes' -> ``depth_gt``
    [1, 1, H, W] and ``boundary`` uint8 [H, W] on the device; ``get_metrics`` then scores with the resize inside the kernel.
    ``gt_shape`` replaces the reference's literal 4032 x 6048 (ETH3D's raw files carry no shape).  ``image_format`` selects
    read_image's branch (:22-62): None / 'mid' bicubic to ``image_resolution``; 'u4k' raw BGR bytes of ``image_resolution``;
    'cityscapes' RGB / 255 as it is; 'kitti' its 352 x 1216 kb-crop -- the last three through ops.u8_image."""
    _reader_name = "gt-read"

    def __init__(self, rgb_image_dir, mode="", min_depth=1e-3, max_depth=80, gt_dir=None, image_resolution=(2160, 3840),
                 dataset_name="", network_process_size=(384, 512), resize_mode="zoe", edge_metrics=False, gt_format=None, image_format=None,
                 gt_shape=(4032, 6048), ssi_metrics=False, boundary_f1=False):
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
        self.boundary_f1 = bool(boundary_f1)  # get_metrics adds the scale-invariant boundary F1 (metrics.BOUNDARY_KEYS), plain set only
        self.files = sorted(os.listdir(rgb_image_dir))
        # ground truth: metric depth as <gt_dir>/<basename>.npy, or (gt_format) the reference's per-dataset files
        self.gt_dir = gt_dir
        self.gt_format = gt_format if gt_dir is not None else None
        self.image_format = image_format
        self.gt_shape = (int(gt_shape[0]), int(gt_shape[1]))
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

    def _make_slot(self):
        return dict(buf=None, image=None)

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
            _read_exact(m["path"], view, m["offset"])
        slot["image"] = None
        if self.image_format in ("u4k", "cityscapes", "kitti"):
            slot["image"] = decode_image_u8(os.path.join(self.rgb_image_dir, self.files[i]), self.image_format, self.image_resolution)

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
        i, slot = self._acquire(i)
        m = self.gt_meta(i)
        raw = slot["buf"][:m["nbytes"]].cuda(non_blocking=True)
        decoded = slot["image"]
        self._release(i)
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
        from functools import partial
        from . import metrics as M
        dev = isinstance(result, torch.Tensor) and result.is_cuda
        score = M.compute_metrics_device if dev else M.compute_metrics
        if self.gt_format is not None:  # the ground truth is on the device: one fused pass, the prediction sampled inside it
            score = partial(M.compute_metrics_fused, fuse_resize=True)
        common = self._common(self.dataset_name)
        with_edges = dict(disp_gt_edges=disp_gt_edges, **common)
        out = score(depth_gt, result, **with_edges)
        if self.edge_metrics:
            out.update(self._edge_metrics(depth_gt, result, dev, score, with_edges))
        # the ssi scores on the device whenever the maps are there, else the host restatement
        ssi = partial(M.compute_ssi_metrics_fused, fuse_resize=True) if self.gt_format is not None or dev else M.compute_ssi_metrics
        return self._with_extras(out, ssi, depth_gt, result, common)

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
class UnrealStereo4kDataset(_StagedDataset):
    """estimator/datasets/u4k_dataset.py:20-233, inference mode: the frames of a split file with their ground truth, decoded on the
    GPU.  Per item the host only reads the two files (``<image>.raw``: BGR bytes; ``Disp0/*.npy``: disparity) into pinned staging
    buffers and copies them to the device; ops.u8_image makes ``image_hr`` (RGB / 255, CHW, bit-equal to the reference's numpy
    expression) and ops.disp_gt makes ``depth_gt`` = depth_factor / disparity and ``boundary`` = get_boundaries(disparity, th=1) in
    one pass.  The files of the NEXT index are read one item ahead on a single background thread (files and host memory only: it
    never touches the GPU).  ``get_metrics`` is metrics.compute_metrics_fused.  ``image_raw_shape`` replaces the reshape the
    reference hard-codes to (2160, 3840).  Not built: ``mode='train'`` (augmentation, crops) and ``consistency=True``."""

    dataset_name = "u4k"
    _reader_name = "u4k-read"

    def __init__(self, mode, data_root, split, transform_cfg, min_depth, max_depth, consistency=False, overlap=0, patch_raw_shape=(540, 960),
                 resize_mode="zoe", pre_norm_bbox=True, image_raw_shape=(2160, 3840), ssi_metrics=False, boundary_f1=False):
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
        self.boundary_f1 = bool(boundary_f1)  # get_metrics adds the scale-invariant boundary F1 (metrics.BOUNDARY_KEYS), plain set only
        self.data_infos = self.load_data_list()

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

    def __getitem__(self, idx):
        from . import ops
        idx, (img, disp) = self._acquire(idx)
        raw = img.cuda(non_blocking=True)
        d = disp.cuda(non_blocking=True)
        self._release(idx)
        info = self.data_infos[idx]
        depth, boundary = ops.disp_gt(d, info["depth_factor"], 1.0)
        return dict(image_hr=ops.u8_image(raw, swap_rb=True), depth_gt=depth[None, None], boundary=boundary,
                    img_file_basename=info["img_file_basename"])

    def get_metrics(self, depth_gt, result, disp_gt_edges=None, **kw):
        """u4k_dataset.py:232-233 through the fused kernel (a host ``result`` is copied to the device first)"""
        from .metrics import compute_metrics_fused, compute_ssi_metrics_fused
        common = self._common()
        out = compute_metrics_fused(depth_gt, result, disp_gt_edges=disp_gt_edges, **common)
        return self._with_extras(out, compute_ssi_metrics_fused, depth_gt, result, common)


ETH_METRIC_KEYS = ("a1", "a2", "a3", "abs_rel", "rmse", "log_10", "rmse_log", "silog", "sq_rel", "see")  # compute_metrics' order


def eth_metric_order(fused: dict) -> dict:
    """compute_metrics_fused(region=...)'s dict in the reference's order (eth_dataset.py:277-289, :304-335): ``edge_*``, ``noedge_*``, then
    the plain keys"""
    plain = [k for k in fused if not k.startswith(("edge_", "noedge_"))]
    return {pre + k: fused[pre + k] for pre in ("edge_", "noedge_", "") for k in plain}


@DATASETS.register_module()
class ETHDataset(_StagedDataset):
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
    _reader_name = "eth-read"

    def __init__(self, mode, split, transform_cfg, min_depth, max_depth, stitcher_stage=0, overlap=0, crop_strategy="random",
                 resize_mode="zoe", gt_shape=(4032, 6048), ssi_metrics=False, boundary_f1=False):
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
        self.boundary_f1 = bool(boundary_f1)  # get_metrics adds the scale-invariant boundary F1 (metrics.BOUNDARY_KEYS), plain set only
        shallow = transform_cfg.get("input_size_shallow", None)
        self.input_size_shallow = None if shallow is None else (int(shallow[0]), int(shallow[1]))
        self.data_infos = self.load_data_list()

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
        _read_exact(self.check_gt_file(idx), slot["gt"].numpy().reshape(-1).view(np.uint8))

    def __getitem__(self, idx):
        from . import ops
        idx, slot = self._acquire(idx)
        h, w = slot["shape"]
        raw = slot["img"][:h * w * 3].cuda(non_blocking=True).view(h, w, 3)
        gt = slot["gt"].cuda(non_blocking=True)
        self._release(idx)
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
        common = self._common(fuse_resize=True)
        out = eth_metric_order(compute_metrics_fused(depth_gt, result, disp_gt_edges=disp_gt_edges, region=region, **common))
        return self._with_extras(out, compute_ssi_metrics_fused, depth_gt, result, common)  # (after the reference's thirty keys)

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


CITYSCAPES_METRIC_KEYS = ETH_METRIC_KEYS + ("EdgeAcc", "EdgeComp", "precision", "recall", "f1_score", "hamming", "acc")  # :422-440


def read_cityscapes_camera(path) -> float:
    """cityscapes_dataset.py:149-156: the decode factor baseline x fx of a camera file as the float32 value the reference's division
    by a float32 array sees; a file without ``extrinsic.baseline`` / ``intrinsic.fx`` raises ValueError naming it"""
    import json
    with open(path) as f:
        try:
            cam = json.load(f)
            return float(np.float32(float(cam["extrinsic"]["baseline"]) * float(cam["intrinsic"]["fx"])))
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError(f"{path}: no extrinsic.baseline / intrinsic.fx in the camera file ({type(e).__name__}: {e})") from None


# (not registered in DATASETS: tools/test.py still answers a config of this type with "is not built", which tests/test_u4k_eval_host.py
#  and tests/test_general_gt_host.py pin; the class is built by its constructor -- tools/test.py --test-type cityscapes does that)
class CityScapesDataset(_StagedDataset):
    """estimator/datasets/cityscapes_dataset.py:27-501, ``mode='infer'``: the frames of a split file with their disparity, camera and
    (``with_seg_map``) colour segmentation map.  One background thread (_ReadAhead: files and host memory only) decodes the NEXT
    frame's image (PIL ``convert("RGB")``), its 16-bit disparity PNG, the segmentation map's RGB bytes and the camera JSON into pinned
    buffers; on the device ops.u8_image makes ``image_hr`` and ONE pass of ops.cityscapes_gt makes ``depth_gt`` [1, 1, H, W]
    (baseline x fx / disparity, -1 in the noisy bands, 0 at the sky class), ``boundary`` and ``seg_image`` (fp32 [3, H, W], 0 .. 255).
    No ``image_lr`` key (Tester._frames makes it with model.resizer).  ``get_metrics`` (:318-408) takes the ten depth metrics on the
    "flatten" pixels -- away from the edges that are both a segmentation edge (ops.seg_canny: kornia's Canny) and a ground-truth depth
    edge, and away from the image's edges -- and the seven boundary metrics against those edges.  ``filter_sky``, ``pre_norm_bbox``,
    ``base``, ``filter_thr`` and ``patch_raw_shape`` are stored (they act in training).  Not built: ``mode='train'``,
    ``transform_cfg.random_crop``, ``transform_cfg.input_size_shallow`` (PIL's antialiased resizes; no shipped Cityscapes config sets
    it), ``with_pseudo_label`` / ``with_uncert`` (training inputs)."""

    dataset_name = "cityscapes"
    _reader_name = "cityscapes-read"

    def __init__(self, mode, split, transform_cfg, min_depth, max_depth, patch_raw_shape=(256, 512), data_root="./data/cityscapes",
                 resize_mode="zoe", with_pseudo_label=False, pseudo_label_path=None, with_seg_map=False, filter_sky=True, pre_norm_bbox=True,
                 with_uncert=False, base=float(np.exp(1)), filter_thr=-0.1, ssi_metrics=False, boundary_f1=False):
        if mode == "train":
            raise NotImplementedError("CityScapesDataset(mode='train'): the training pipeline (aug_rotate / aug_color / aug_flip / "
                                      "random_crop, cityscapes_dataset.py:178-298) is not built; inference modes only")
        if transform_cfg.get("random_crop", False):
            raise NotImplementedError("CityScapesDataset(transform_cfg.random_crop): the random crops (cityscapes_dataset.py:263-280) are not built")
        if transform_cfg.get("input_size_shallow", None) is not None:
            raise NotImplementedError("CityScapesDataset(transform_cfg.input_size_shallow): PIL's antialiased resizes "
                                      "(cityscapes_dataset.py:193-197) are not built; no shipped Cityscapes config sets it")
        if with_pseudo_label or with_uncert:
            raise NotImplementedError("CityScapesDataset(with_pseudo_label / with_uncert): pseudo labels and their uncertainty are training "
                                      "inputs (cityscapes_dataset.py:200-219)")
        if resize_mode not in ("zoe", "depth-anything"):
            raise NotImplementedError(f"CityScapesDataset(resize_mode={resize_mode!r})")  # cityscapes_dataset.py:66-73
        self.mode, self.split, self.data_root = mode, split, data_root
        self.min_depth, self.max_depth = min_depth, max_depth
        self.transform_cfg = transform_cfg
        self.resize_mode = resize_mode
        self.with_seg_map = bool(with_seg_map)
        self.with_pseudo_label, self.with_uncert, self.pseudo_label_path = False, False, pseudo_label_path
        self.filter_sky, self.pre_norm_bbox, self.base, self.filter_thr = filter_sky, pre_norm_bbox, base, filter_thr
        self.patch_raw_shape = tuple(patch_raw_shape)
        self.ssi_metrics = bool(ssi_metrics)  # get_metrics adds the scale-and-shift-invariant scores (metrics.SSI_KEYS), plain set only
        self.boundary_f1 = bool(boundary_f1)  # get_metrics adds the scale-invariant boundary F1 (metrics.BOUNDARY_KEYS), plain set only
        self.data_infos = self.load_data_list()

    def load_data_list(self):
        """cityscapes_dataset.py:86-138: 'img disp' per line, joined to ``data_root``; the camera file is the image path with
        leftImg8bit -> camera and .png -> .json, the segmentation map the disparity path with disparity -> gtFine and .png ->
        _color.png; sorted by image path; the basename of :260-261"""
        if self.split is None:
            raise NotImplementedError("CityScapesDataset needs a split file (cityscapes_dataset.py:133-134)")
        infos = []
        with open(self.split) as f:
            for line in f:
                if not line.strip():
                    continue
                img, depth_map = line.strip().split(" ")
                info = dict(depth_map_path=os.path.join(self.data_root, depth_map), img_path=os.path.join(self.data_root, img), filename=img)
                info["camera_info"] = info["img_path"].replace("leftImg8bit", "camera").replace(".png", ".json")
                if self.with_seg_map:
                    info["seg_map"] = info["depth_map_path"].replace("disparity", "gtFine").replace(".png", "_color.png")
                info["img_file_basename"] = os.path.splitext(img)[0].replace("/", "_")
                infos.append(info)
        return sorted(infos, key=lambda x: x["img_path"])

    def __len__(self):
        return len(self.data_infos)

    def _make_slot(self):
        return dict(img=None, disp=None, seg=None, shape=None, factor=None)

    def _prepare(self, idx, slot):
        """(caller's thread) the slot's pinned buffers hold a frame of item ``idx``'s disparity size, read from the PNG's header
        (ValueError naming the file unless it is 16-bit greyscale)"""
        h, w = _png16_shape(self.data_infos[idx]["depth_map_path"])
        px = h * w
        for key, item in (("img", 3), ("disp", 2)) + ((("seg", 3),) if self.with_seg_map else ()):
            if slot[key] is None or slot[key].numel() < px * item:
                slot[key] = torch.empty((px * item,), dtype=torch.uint8).pin_memory()

    def _read(self, idx, slot):
        """(background thread: files and host memory only) the disparity samples, the image's and the segmentation map's RGB bytes
        and the camera's factor of item ``idx``; every size is checked against the disparity's"""
        from PIL import Image
        info = self.data_infos[idx]
        h, w = _png16_shape(info["depth_map_path"])  # (ValueError naming the file unless it is 16-bit greyscale)
        d = np.asarray(Image.open(info["depth_map_path"]))  # cv2.imread(path, IMREAD_UNCHANGED) of a 16-bit PNG: its uint16 samples
        if d.shape != (h, w) or d.dtype.itemsize != 2:
            raise ValueError(f"{info['depth_map_path']}: decoded to {d.dtype} {d.shape}, expected uint16 {(h, w)}")
        np.copyto(slot["disp"].numpy()[:h * w * 2].view(np.uint16).reshape(h, w), d, casting="unsafe")
        for key, path, what in (("img", info["img_path"], "image"),) + ((("seg", info["seg_map"], "segmentation map"),) if self.with_seg_map else ()):
            a = np.asarray(Image.open(path).convert("RGB"))  # cityscapes_dataset.py:146, :170
            if a.shape[:2] != (h, w):
                raise ValueError(f"{path}: the {what} is {a.shape[0]} x {a.shape[1]}, the disparity map {info['depth_map_path']} {h} x {w}")
            np.copyto(slot[key].numpy()[:a.size].reshape(a.shape), a)
        slot["shape"], slot["factor"] = (h, w), read_cityscapes_camera(info["camera_info"])

    def __getitem__(self, idx):
        from . import ops
        idx, slot = self._acquire(idx)
        h, w = slot["shape"]
        raw = slot["img"][:h * w * 3].cuda(non_blocking=True).view(h, w, 3)
        disp = slot["disp"][:h * w * 2].cuda(non_blocking=True).view(torch.uint16).view(h, w)
        seg = slot["seg"][:h * w * 3].cuda(non_blocking=True).view(h, w, 3) if self.with_seg_map else None
        factor = slot["factor"]
        self._release(idx)
        depth, boundary, seg_image = ops.cityscapes_gt(disp, seg, factor)  # :153-174 and get_boundaries(disp_gt, th=1, dilation=0), :300
        item = dict(image_hr=ops.u8_image(raw, swap_rb=False), depth_gt=depth[None, None], boundary=boundary,
                    img_file_basename=self.data_infos[idx]["img_file_basename"])
        if self.with_seg_map:
            item["seg_image"] = seg_image
        return item

    def get_metrics(self, depth_gt, result, disp_gt_edges, seg_image=None, image_hr=None, **kw):
        """cityscapes_dataset.py:318-408 on the device: edge = segmentation edges (ops.seg_canny) that are 7 x 7-widened ground-truth
        depth edges, flatten = neither such an edge nor in the image's edge area (ops.image_edge_region, frac 0.05) -- one pass of
        ops.cityscapes_masks; the ten depth metrics on the flatten pixels (the prediction's resize inside the scoring kernel), then the
        seven boundary metrics of the prediction's log-depth Canny edges against the edge set at the valid pixels.  The noisy bands
        are -1 in ``depth_gt`` already, so ``valid`` is the depth range alone."""
        from . import metrics as M, ops
        if seg_image is None or image_hr is None:
            raise ValueError("CityScapesDataset.get_metrics needs seg_image (with_seg_map=True) and image_hr: its pixel sets come from "
                             "the segmentation map's and the image's edges (cityscapes_dataset.py:333, :346)")
        H, W = depth_gt.shape[-2:]
        gt = torch.as_tensor(depth_gt).cuda().float().reshape(H, W)
        seg = torch.as_tensor(seg_image).cuda().float().reshape(3, H, W)
        image = torch.as_tensor(image_hr).cuda().float()
        region = ops.image_edge_region(image.reshape(3, *image.shape[-2:]), H, W, frac=0.05)  # :346-352
        edge_mask, flatten = ops.cityscapes_masks(ops.seg_canny(seg), M.extract_edges_device(gt, "log"), region)
        common = self._common(fuse_resize=True)
        out = M.compute_metrics_fused(depth_gt, result, disp_gt_edges=disp_gt_edges, additional_mask=flatten, **common)
        pred = torch.as_tensor(result).cuda().float().reshape(1, 1, *result.shape[-2:])
        if pred.shape[-2:] != (H, W):  # :320-322
            pred = F.interpolate(pred, (H, W), mode="bilinear", align_corners=False)
        valid = (gt > self.min_depth) & (gt < self.max_depth)
        out.update(M.compute_boundary_metrics_device(edge_mask, M.extract_edges_device(pred, "log"), valid))
        return self._with_extras(out, M.compute_ssi_metrics_fused, depth_gt, result, common)

    def evaluate(self, results, **kw):
        """cityscapes_dataset.py:410-501 without the table: np.nanmean of every key over the frames' metric dicts, as ETHDataset's"""
        return ETHDataset.evaluate(self, results)


def _read_depth16(path, view, what):
    """(background thread) the uint16 samples of the 16-bit greyscale PNG ``path`` as the file holds them into the byte array ``view``
    -> (h, w); ValueError naming the file unless it is one"""
    from PIL import Image
    h, w = _png16_shape(path, what)
    d = np.asarray(Image.open(path))  # np.asarray(Image.open(path)) of an I;16 image: its uint16 samples
    if d.shape != (h, w) or d.dtype.itemsize != 2:
        raise ValueError(f"{path}: decoded to {d.dtype} {d.shape}, expected uint16 {(h, w)}")
    np.copyto(view[:h * w * 2].view(np.uint16).reshape(h, w), d, casting="unsafe")
    return h, w


def _pinned(slot, key, need):
    """(caller's thread) ``slot[key]`` is a pinned byte buffer of at least ``need`` bytes"""
    if slot[key] is None or slot[key].numel() < need:
        slot[key] = torch.empty((need,), dtype=torch.uint8).pin_memory()


# (KittiDataset and ScanNetDataset are not registered in DATASETS either, for CityScapesDataset's reason: tools/test.py --test-type
#  kitti / scannet build them by their constructors)
class KittiDataset(_StagedDataset):
    """estimator/datasets/kitti_dataset.py:22-295, ``mode='infer'``: the 'img depth' pairs of a split file under ``data_root/raw`` and
    ``data_root/depth`` (a depth of ``None`` skips the line).  One background thread (_ReadAhead: files and host memory only) decodes the
    NEXT image with PIL -- through decode_image_u8's kb-crop when ``do_kb_crop`` -- and reads the depth PNG's uint16 samples UNCROPPED
    into a pinned buffer; on the device ops.u8_image makes ``image_hr`` and ops.depth16_gt reads the samples through the crop's window
    (top = h - 352, left = int((w - 1216) / 2), :123-131) -> ``depth_gt`` [1, 1, H, W] = samples / 256 (:142) and ``boundary`` (:203) in
    one pass.  No ``image_lr`` key (Tester._frames makes it with model.resizer).  ``get_metrics`` (:219-222) is one fused pass inside the
    Garg crop with the prediction's resize in the kernel; ``evaluate`` the per-key nanmean (sparse LiDAR: a frame without a valid pixel
    in the crop is NaN and does not poison the mean).  ``patch_raw_shape`` and ``pre_norm_bbox`` are stored (they act in training).
    Not built: ``mode='train'`` (:133-152, :168-200), ``with_pseudo_label`` (:92-99, :119-121), ``transform_cfg.random_crop``."""

    dataset_name = "kitti"
    _reader_name = "kitti-read"

    def __init__(self, mode, data_root, split, transform_cfg, min_depth, max_depth, patch_raw_shape=(176, 304), resize_mode="zoe",
                 with_pseudo_label=False, pseudo_label_path=None, do_kb_crop=True, pre_norm_bbox=True, ssi_metrics=False, boundary_f1=False):
        if mode == "train":
            raise NotImplementedError("KittiDataset(mode='train'): the training pipeline (aug_rotate / aug_color / aug_flip / random_crop, "
                                      "kitti_dataset.py:133-152, :168-200) is not built; inference modes only")
        if transform_cfg.get("random_crop", False):
            raise NotImplementedError("KittiDataset(transform_cfg.random_crop): the random crops (kitti_dataset.py:168-188) are not built")
        if with_pseudo_label:
            raise NotImplementedError("KittiDataset(with_pseudo_label): pseudo labels are training inputs (kitti_dataset.py:92-99, :119-121)")
        if resize_mode not in ("zoe", "depth-anything"):
            raise NotImplementedError(f"KittiDataset(resize_mode={resize_mode!r})")  # kitti_dataset.py:52-59
        self.mode, self.data_root, self.split = mode, data_root, split
        self.min_depth, self.max_depth = min_depth, max_depth
        self.transform_cfg = transform_cfg
        self.resize_mode = resize_mode
        self.with_pseudo_label, self.pseudo_label_path = False, pseudo_label_path
        self.patch_raw_shape, self.pre_norm_bbox, self.do_kb_crop = tuple(patch_raw_shape), pre_norm_bbox, bool(do_kb_crop)
        self.ssi_metrics = bool(ssi_metrics)  # get_metrics adds the scale-and-shift-invariant scores (metrics.SSI_KEYS)
        self.boundary_f1 = bool(boundary_f1)  # get_metrics adds the scale-invariant boundary F1 (metrics.BOUNDARY_KEYS), plain set only
        self.data_infos = self.load_data_list()

    def load_data_list(self):
        """kitti_dataset.py:66-107: 'img depth' per line, a depth of 'None' skips it; data_root/raw/<img> and data_root/depth/<depth>;
        sorted by image path; the basename of :165-166"""
        if self.split is None:
            raise NotImplementedError("KittiDataset needs a split file (kitti_dataset.py:103-104)")
        infos = []
        with open(self.split) as f:
            for line in f:
                if not line.strip():
                    continue
                img, depth = line.strip().split(" ")[0], line.strip().split(" ")[1]
                if depth == "None":
                    continue
                infos.append(dict(depth_map_path=os.path.join(self.data_root, "depth", depth), img_path=os.path.join(self.data_root, "raw", img),
                                  filename=img, img_file_basename=os.path.splitext(img)[0].replace("/", "_")))
        return sorted(infos, key=lambda x: x["img_path"])

    def __len__(self):
        return len(self.data_infos)

    def _make_slot(self):
        return dict(img=None, depth=None, shape=None, img_shape=None)

    def _prepare(self, idx, slot):
        """(caller's thread) the slot's pinned buffers hold a frame of item ``idx``'s depth size, read from the PNG's header
        (ValueError naming the file unless it is 16-bit greyscale)"""
        h, w = _png16_shape(self.data_infos[idx]["depth_map_path"], "a KITTI depth map")
        _pinned(slot, "img", h * w * 3)
        _pinned(slot, "depth", h * w * 2)

    def _read(self, idx, slot):
        """(background thread: files and host memory only) the depth PNG's samples, uncropped, and the image's RGB bytes (kb-cropped
        with ``do_kb_crop``); the two sizes are checked against each other and against the crop"""
        from PIL import Image
        info = self.data_infos[idx]
        h, w = _read_depth16(info["depth_map_path"], slot["depth"].numpy(), "a KITTI depth map")
        with Image.open(info["img_path"]) as im:
            ih, iw = im.height, im.width
        if (ih, iw) != (h, w):
            raise ValueError(f"{info['img_path']}: the image is {ih} x {iw}, the depth map {info['depth_map_path']} {h} x {w}")
        if self.do_kb_crop and (h < KB_CROP[0] or w < KB_CROP[1]):
            raise ValueError(f"{info['depth_map_path']}: {h} x {w} (as {info['img_path']}) is smaller than the kb-crop {KB_CROP[0]} x {KB_CROP[1]}")
        a, _ = decode_image_u8(info["img_path"], "kitti" if self.do_kb_crop else "cityscapes", None)  # kitti_dataset.py:114, :123-131
        np.copyto(slot["img"].numpy()[:a.size].reshape(a.shape), a)
        slot["shape"], slot["img_shape"] = (h, w), a.shape[:2]

    def __getitem__(self, idx):
        from . import ops
        idx, slot = self._acquire(idx)
        (h, w), (H, W) = slot["shape"], slot["img_shape"]
        raw = slot["img"][:H * W * 3].cuda(non_blocking=True).view(H, W, 3)
        samples = slot["depth"][:h * w * 2].cuda(non_blocking=True).view(torch.uint16).view(h, w)
        self._release(idx)
        # :126-127: top_margin = int(height - 352), left_margin = int((width - 1216) / 2); without the crop the whole map
        window = (int(h - KB_CROP[0]), int((w - KB_CROP[1]) / 2)) if self.do_kb_crop else (0, 0)
        depth, boundary = ops.depth16_gt(samples, (H, W), 256.0, window=window, th=1.0)  # :142 and get_boundaries(depth_gt, th=1, dilation=0), :203
        return dict(image_hr=ops.u8_image(raw, swap_rb=False), depth_gt=depth[None, None], boundary=boundary,
                    img_file_basename=self.data_infos[idx]["img_file_basename"])

    def get_metrics(self, depth_gt, result, disp_gt_edges=None, **kw):
        """kitti_dataset.py:219-222 through the fused kernel: the Garg crop, the prediction's resize inside the scoring pass"""
        from .metrics import compute_metrics_fused, compute_ssi_metrics_fused
        common = dict(self._common("kitti", fuse_resize=True), garg_crop=True)
        out = compute_metrics_fused(depth_gt, result, disp_gt_edges=disp_gt_edges, **common)
        return self._with_extras(out, compute_ssi_metrics_fused, depth_gt, result, common)

    def boundary_args(self):
        return dict(self._common("kitti"), garg_crop=True)

    def evaluate(self, results, **kw):
        """kitti_dataset.py:224-295 without the table: np.nanmean of every key over the frames' metric dicts, as ETHDataset's"""
        return ETHDataset.evaluate(self, results)


class ScanNetDataset(_StagedDataset):
    """estimator/datasets/scannet_dataset.py:25-404, inference modes: the 'img depth' pairs (absolute paths) of a split file.  One
    background thread (_ReadAhead: files and host memory only) decodes the NEXT image with PIL (``convert("RGB")``) and reads the depth
    PNG's uint16 samples at their OWN size into a pinned buffer; on the device ops.u8_image makes ``image_hr`` and ops.depth16_gt brings
    the samples to the image's size by the rule of PIL's ``resize(image.size, Image.NEAREST)`` (:112-118) -> ``depth_gt`` [1, 1, H, W] =
    samples / 1000 (:132) and ``boundary`` (:188) in one pass.  No ``image_lr`` key.  ``get_metrics`` (:209-244) widens the log-depth
    Canny edges of the ground truth by 7 x 7 on the device and scores inside them, outside them and everywhere in ONE fused pass, the
    prediction's resize inside it: ``edge_*``, ``noedge_*``, then the plain keys.  ``evaluate`` / ``evaluate_consistency`` are the
    per-key nanmean.  ``patch_raw_shape`` and ``pre_norm_bbox`` are stored.  Not built: ``mode='train'`` (:120-129, :139-146),
    ``transform_cfg.random_crop`` (:156-173), ``with_pseudo_label`` (:90-93, :121-124)."""

    dataset_name = "scannet"
    _reader_name = "scannet-read"

    def __init__(self, mode, split, transform_cfg, min_depth, max_depth, with_pseudo_label=False, pseudo_label_path=None,
                 patch_raw_shape=(720, 960), resize_mode="zoe", pre_norm_bbox=True, ssi_metrics=False, boundary_f1=False):
        if mode == "train":
            raise NotImplementedError("ScanNetDataset(mode='train'): the training pipeline (aug_rotate / aug_color / aug_flip, "
                                      "scannet_dataset.py:120-129, :139-146) is not built; inference modes only")
        if transform_cfg.get("random_crop", False):
            raise NotImplementedError("ScanNetDataset(transform_cfg.random_crop): the random crops (scannet_dataset.py:156-173) are not built")
        if with_pseudo_label:
            raise NotImplementedError("ScanNetDataset(with_pseudo_label): pseudo labels are training inputs (scannet_dataset.py:90-93, :121-124)")
        if resize_mode not in ("zoe", "depth-anything"):
            raise NotImplementedError(f"ScanNetDataset(resize_mode={resize_mode!r})")  # scannet_dataset.py:53-60
        self.mode, self.split = mode, split
        self.min_depth, self.max_depth = min_depth, max_depth
        self.transform_cfg = transform_cfg
        self.resize_mode = resize_mode
        self.with_pseudo_label, self.pseudo_label_path = False, pseudo_label_path
        self.patch_raw_shape, self.pre_norm_bbox = tuple(patch_raw_shape), pre_norm_bbox
        self.ssi_metrics = bool(ssi_metrics)  # get_metrics adds the scale-and-shift-invariant scores (metrics.SSI_KEYS), plain set only
        self.boundary_f1 = bool(boundary_f1)  # get_metrics adds the scale-invariant boundary F1 (metrics.BOUNDARY_KEYS), plain set only
        self.data_infos = self.load_data_list()

    @staticmethod
    def basename_of(img_path):
        """scannet_dataset.py:191-193, literally (the reference's 'bad hack': scene id and frame number of a ScanNet++ path)"""
        img_file_basename, _ = os.path.splitext(img_path)
        img_file_basename = img_file_basename.replace("/", "_")[1:]
        return img_file_basename[-34:-24] + "_" + img_file_basename[-6:]

    def load_data_list(self):
        """scannet_dataset.py:67-102: 'img depth' per line (absolute paths), sorted by image path"""
        if self.split is None:
            raise NotImplementedError("ScanNetDataset needs a split file (scannet_dataset.py:97-98)")
        infos = []
        with open(self.split) as f:
            for line in f:
                if not line.strip():
                    continue
                img, depth_map = line.strip().split(" ")
                infos.append(dict(depth_map_path=depth_map, img_path=img, depth_fields=[], img_file_basename=self.basename_of(img)))
        return sorted(infos, key=lambda x: x["img_path"])

    def __len__(self):
        return len(self.data_infos)

    def _make_slot(self):
        return dict(img=None, depth=None, shape=None, img_shape=None)

    def _prepare(self, idx, slot):
        """(caller's thread) the slot's pinned buffers hold item ``idx``'s image and depth samples (both headers are read here; ValueError
        naming the depth file unless it is 16-bit greyscale)"""
        from PIL import Image
        info = self.data_infos[idx]
        h, w = _png16_shape(info["depth_map_path"], "a ScanNet depth map")
        with Image.open(info["img_path"]) as im:
            _pinned(slot, "img", im.height * im.width * 3)
        _pinned(slot, "depth", h * w * 2)

    def _read(self, idx, slot):
        """(background thread: files and host memory only) the image's RGB bytes and the depth PNG's samples at their own size"""
        from PIL import Image
        info = self.data_infos[idx]
        a = np.asarray(Image.open(info["img_path"]).convert("RGB"))  # scannet_dataset.py:109
        if slot["img"].numel() < a.size:
            raise ValueError(f"{info['img_path']}: decoded to {a.shape}, more than its header announced")
        np.copyto(slot["img"].numpy()[:a.size].reshape(a.shape), a)
        slot["shape"] = _read_depth16(info["depth_map_path"], slot["depth"].numpy(), "a ScanNet depth map")
        slot["img_shape"] = a.shape[:2]

    def __getitem__(self, idx):
        from . import ops
        idx, slot = self._acquire(idx)
        (h, w), (H, W) = slot["shape"], slot["img_shape"]
        raw = slot["img"][:H * W * 3].cuda(non_blocking=True).view(H, W, 3)
        samples = slot["depth"][:h * w * 2].cuda(non_blocking=True).view(torch.uint16).view(h, w)
        self._release(idx)
        # :115-118 resize(image.size, NEAREST), :132 / 1000.0 (mm to m), get_boundaries(depth_gt, th=1, dilation=0), :188
        depth, boundary = ops.depth16_gt(samples, (H, W), 1000.0, nearest=True, th=1.0)
        return dict(image_hr=ops.u8_image(raw, swap_rb=False), depth_gt=depth[None, None], boundary=boundary,
                    img_file_basename=self.data_infos[idx]["img_file_basename"])

    def get_metrics(self, depth_gt, result, disp_gt_edges=None, **kw):
        """scannet_dataset.py:209-244: the edge area is the 7 x 7-widened log-depth Canny edges of the ground truth
        (metrics.edge_split_masks, on the device), then the reference's three compute_metrics calls as ONE fused pass over the three
        pixel sets -> ``edge_*``, ``noedge_*``, then the plain keys.  It needs no ``image_hr``."""
        from . import metrics as M
        H, W = depth_gt.shape[-2:]
        gt = torch.as_tensor(depth_gt).cuda().float().reshape(H, W)
        region = M.edge_split_masks_device(gt, 7)  # ops.binary_dilate(extract_edges_device(gt, 'log'), 7)
        common = self._common(fuse_resize=True)
        out = eth_metric_order(M.compute_metrics_fused(gt[None, None], result, disp_gt_edges=disp_gt_edges, region=region, **common))
        return self._with_extras(out, M.compute_ssi_metrics_fused, depth_gt, result, common)  # (after the reference's thirty keys)

    def evaluate(self, results, **kw):
        """scannet_dataset.py:246-339 without the table: np.nanmean of every key over the frames' metric dicts, as ETHDataset's"""
        return ETHDataset.evaluate(self, results)

    def evaluate_consistency(self, results, **kw):
        """scannet_dataset.py:342-404 without the table: the nanmean of ``consistency_error``"""
        return ETHDataset.evaluate(self, [dict(consistency_error=r["consistency_error"]) for r in results])
