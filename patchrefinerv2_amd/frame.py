"""How a frame is executed: tiling -> per-patch networks -> overlap blend, all on the device.  ``FrameDriver`` is the base of the
tiling models (models.py: what a model is -- its networks, ``infer_forward`` / ``coarse_forward``, checkpoints).

What differs from the reference on purpose (results identical):
  * the complete tile list is drawn up-front (consuming Python's ``random`` in the reference's
    order) so patches can be batched / sharded freely -- per-patch results do not depend on batching;
  * the blend state stays on the device (one D2H at the end) instead of a CPU map per tile;
  * no ``feat.repeat(K)``: ROI gathers read the single coarse pyramid;
  * no ``torch.cuda.empty_cache()`` per mini-batch.
"""
from __future__ import annotations

import random
from typing import List

import numpy as np
import torch

from . import ops
from .ops import Feat


# ------------------------------------------------------------------------------------------------
# host-side pieces of the path: blend mask + resize target (tiny, once per frame / model)
# ------------------------------------------------------------------------------------------------
def _gaussian_kernel1d(ksize: int, sigma: float) -> np.ndarray:
    c = (ksize - 1) * 0.5
    i = np.arange(ksize, dtype=np.float64)
    k = np.exp(-((i - c) ** 2) / (2.0 * float(sigma) ** 2))
    return (k / k.sum()).astype(np.float32)


def generatemask(size, border: float = 0.1) -> np.ndarray:
    """estimator/models/utils.py:51-60 with cv2.GaussianBlur restated in numpy (separable Gaussian,
    BORDER_REFLECT_101).  Host logic exactly as in the reference (it runs cv2 on the CPU, once per
    mode per frame); the zero band of the box is wider than the half kernel on every shape of the
    path, so the border mode never matters."""
    h, w = int(size[0]), int(size[1])
    mask = np.zeros((h, w), dtype=np.float32)
    sigma = int(h / 16)
    k_size = int(2 * np.ceil(2 * int(h / 16)) + 1)
    mask[int(border * h): h - int(border * h), int(border * w): w - int(border * w)] = 1
    k = _gaussian_kernel1d(k_size, sigma)
    r = k_size // 2
    pad = np.pad(mask, ((0, 0), (r, r)), mode="reflect")
    tmp = np.zeros_like(mask)
    for i in range(k_size):
        tmp += k[i] * pad[:, i:i + w]
    pad = np.pad(tmp, ((r, r), (0, 0)), mode="reflect")
    out = np.zeros_like(mask)
    for i in range(k_size):
        out += k[i] * pad[i:i + h, :]
    out = (out - out.min()) / (out.max() - out.min())
    return out.astype(np.float32)


_MASK_CACHE = {}


def blend_mask(size, border, add, device) -> torch.Tensor:
    key = (int(size[0]), int(size[1]), float(border), float(add), str(device))
    if key not in _MASK_CACHE:
        _MASK_CACHE[key] = torch.from_numpy(generatemask(size, border) + np.float32(add)).to(device)
    return _MASK_CACHE[key]


class DeviceRunningAverageMap:
    """RunningAverageMap (estimator/models/utils.py:22-49) resident in HBM.  ``frames``: B maps [B, h, w], each pass step one launch
    for all of them (preds [B, k, ph, pw] / tiles [B, k, 2]: the pass's slice of every frame).  ``stats``: two more maps, ``m2`` (the
    weighted sum of squared deviations of the overlapping predictions) and ``ntl`` (tiles covering the pixel), kept by the
    prv2_blend_*_stats kernels; avg / cnt are bit-identical to the map without them."""

    def __init__(self, h, w, device, frames=None, stats=False):
        shape = (h, w) if frames is None else (frames, h, w)
        self.avg = torch.zeros(shape, device=device)
        self.cnt = torch.zeros(shape, device=device)
        self.m2 = torch.zeros(shape, device=device) if stats else None
        self.ntl = torch.zeros(shape, device=device) if stats else None

    def paste(self, preds, mask, tiles, th, tw):
        if self.m2 is not None:
            return ops.blend_paste_stats(self.avg, self.cnt, self.m2, self.ntl, preds, mask, tiles, th, tw)
        if self.avg.dim() == 3:
            return ops.blend_paste_frames(self.avg, self.cnt, preds, mask, tiles, th, tw)
        ops.blend_paste(self.avg, self.cnt, preds, mask, tiles, th, tw)

    def update(self, preds, mask, tiles, th, tw):
        if self.m2 is not None:
            return ops.blend_update_stats(self.avg, self.cnt, self.m2, self.ntl, preds, mask, tiles, th, tw)
        if self.avg.dim() == 3:
            return ops.blend_update_frames(self.avg, self.cnt, preds, mask, tiles, th, tw)
        ops.blend_update(self.avg, self.cnt, preds, mask, tiles, th, tw)

    def resize(self, resolution):
        if self.m2 is not None:
            self.avg, self.cnt, self.m2, self.ntl = ops.blend_resize_stats(self.avg, self.cnt, self.m2, self.ntl, int(resolution[0]),
                                                                           int(resolution[1]))
            return
        self.avg, self.cnt = ops.blend_resize(self.avg, self.cnt, int(resolution[0]), int(resolution[1]))

    def stats_maps(self):
        """(uncertainty, count_map) of the current state, shaped like ``avg``: the weighted standard deviation of the overlapping tile
        predictions (sqrt(max(m2, 0) / cnt), 0 where cnt == 0) and the number of tiles covering the pixel"""
        return ops.blend_uncertainty(self.cnt, self.m2), self.ntl


class FrameDriver:
    """The tile planner, the frame drivers (one GPU, B frames, patch-sharded), the hipGraph capture and the next frame's coarse prefetch.
    Mixed into a model that has ``patch_process_shape``, ``tile_cfg``, ``blend_border``, ``needs_coarse``, the crop normalisation
    (``crop_channels`` / ``crop_mean`` / ``crop_std``), ``infer_forward`` and, with ``needs_coarse``, ``coarse_forward``."""

    def random_calls(self, cai_mode: str, process_num: int) -> int:
        """random_tile calls of an r<N> mode: N // process_num (patchrefinerplus.py:517-520, patchrefiner.py:388-391)"""
        return int(cai_mode[1:]) // process_num

    # -- BaselinePretrain.prepare_tile_cfg (baseline_pretrain.py:96-124) ---------------------------
    def prepare_tile_cfg(self, image_raw_shape, patch_split_num):
        ph, pw = self.patch_process_shape
        sh, sw = patch_split_num
        if image_raw_shape[0] % (2 * sh) or image_raw_shape[1] % (2 * sw):
            # the reference only documents this (docs/user_infer.md:16, asserts commented out)
            raise ValueError(f"image_raw_shape {list(image_raw_shape)} must be divisible by 2*patch_split_num "
                             f"{[2 * sh, 2 * sw]}")
        raw = (image_raw_shape[0] // sh, image_raw_shape[1] // sw)
        return dict(patch_split_num=list(patch_split_num), patch_reensemble_shape=(ph * sh, pw * sw),
                    patch_raw_shape=raw, image_raw_shape=list(image_raw_shape),
                    raw_h_split_point=[int(raw[0] * i) for i in range(sh)],
                    raw_w_split_point=[int(raw[1] * i) for i in range(sw)])

    # -- tile plan --------------------------------------------------------------------------------
    def plan_tiles(self, tile_cfg, cai_mode: str, process_num: int):
        """Every tile of the frame, in the reference's execution order.  Returns a list of passes
        ``dict(kind, raw=[(h,w)], proc=[(h,w)])``; kind 'init' | 'grid' | 'random'."""
        H, W = tile_cfg["image_raw_shape"]
        rh, rw = tile_cfg["patch_raw_shape"]
        RH, RW = tile_cfg["patch_reensemble_shape"]
        ph, pw = self.patch_process_shape

        def grid(off, offp):
            assert off[0] >= 0 and off[1] >= 0
            hs = [rh * i + off[0] for i in range((H - off[0]) // rh)]
            ws = [rw * i + off[1] for i in range((W - off[1]) // rw)]
            hps = [ph * i + offp[0] for i in range((RH - offp[0]) // ph)]
            wps = [pw * i + offp[1] for i in range((RW - offp[1]) // pw)]
            return [(h, w) for h in hs for w in ws], [(h, w) for h in hps for w in wps]

        passes = []
        r, p = grid((0, 0), (0, 0))
        passes.append(dict(kind="init", raw=r, proc=p))
        if cai_mode == "m2" or cai_mode[0] == "r":
            for off, offp in (((0, rw // 2), (0, pw // 2)), ((rh // 2, 0), (ph // 2, 0)),
                              ((rh // 2, rw // 2), (ph // 2, pw // 2))):
                r, p = grid(off, offp)
                if not r:
                    # the reference dies here too (torch.stack of an empty crop list, baseline_pretrain.py:280)
                    raise RuntimeError(f"cai_mode {cai_mode!r} needs patch_split_num >= 2 on both axes (got "
                                       f"{tile_cfg['patch_split_num']}): a half-offset pass would be empty")
                passes.append(dict(kind="grid", raw=r, proc=p))
        elif cai_mode != "m1":
            raise ValueError(f"unknown cai_mode {cai_mode!r} (expected m1, m2 or r<N>)")
        if cai_mode[0] == "r":
            tiles = []
            for _ in range(self.random_calls(cai_mode, process_num)):
                # baseline_pretrain.py:160-161: process_num h-starts, then ONE w-start, per call
                hs = [random.randint(0, H - rh - 1) for _ in range(process_num)]
                ws = random.randint(0, W - rw - 1)
                tiles += [(h, ws) for h in hs]
            passes.append(dict(kind="random", raw=tiles, proc=tiles))
        return passes

    def plan_frames(self, tile_cfg, cai_mode: str, process_num: int, n_frames: int, frame_seeds=None):
        """The tile plans of ``n_frames`` frames, in frame order: Python's ``random`` is consumed exactly as by ``n_frames``
        sequential ``plan_tiles`` calls, and with ``frame_seeds`` it is reseeded with ``frame_seeds[f]`` right before frame f's
        plan (what a per-frame ``random.seed`` of the caller's loop does).  Host only."""
        if frame_seeds is not None and len(frame_seeds) != n_frames:
            raise ValueError(f"frame_seeds has {len(frame_seeds)} entries for {n_frames} frames")
        plans = []
        for f in range(n_frames):
            if frame_seeds is not None:
                random.seed(frame_seeds[f])
            plans.append(self.plan_tiles(tile_cfg, cai_mode, process_num))
        return plans

    # -- coarse pyramid ROI + crops for a set of tiles ---------------------------------------------
    def _boxes(self, tiles, tile_cfg) -> np.ndarray:
        """bboxs * bboxs_feat_factor in float32 (baseline_pretrain.py:289-296)."""
        H, W = tile_cfg["image_raw_shape"]
        rh, rw = tile_cfg["patch_raw_shape"]
        ph, pw = self.patch_process_shape
        bb = np.array([[w, h, w + rw, h + rh] for h, w in tiles], dtype=np.int32).astype(np.float32)
        fac = np.array([1 / W * pw, 1 / H * ph, 1 / W * pw, 1 / H * ph], dtype=np.float32)
        return (bb * fac[None]).astype(np.float32)

    def _prepare_batch(self, image_hr_chw, t_dev, boxes_dev, tile_cfg, coarse_feats: List[Feat], coarse_depth: Feat):
        """t_dev: int32 [k, 2] (h_start, w_start) of the batch's tiles, boxes_dev: fp32 [k, 4] lr-frame ROI boxes, on the device.
        B frames: image [B, 3, H, W], t_dev [k, 3] = (frame, h, w), boxes_dev [k, 5] = (frame, x1, y1, x2, y2), pyramid of B maps."""
        dev = image_hr_chw.device
        ph, pw = self.patch_process_shape
        rh, rw = tile_cfg["patch_raw_shape"]
        K = t_dev.shape[0]
        crops = Feat.alloc(K, ph, pw, self.crop_channels, dev, pad_to=4)
        ops.crop_resize(image_hr_chw, t_dev, rh, rw, ph, pw, self.crop_mean, self.crop_std, crops)
        if not self.needs_coarse:
            return crops, None, None
        # roi_align(feat, boxes, (h, w), h / ph, aligned=True) per level (patchrefinerplus.py:268-276)
        # (not materialised: each level is gathered straight into the concat buffers that consume it -- ops.RoiSource)
        rois = [ops.RoiSource(f, boxes_dev, f.h / ph, f.h, f.w) for f in coarse_feats]
        depth_roi = ops.roi_align(coarse_depth, boxes_dev, coarse_depth.h / ph, coarse_depth.h, coarse_depth.w,
                                  out=Feat(torch.empty((K, coarse_depth.h, coarse_depth.w, 1), device=dev)))
        return crops, rois, depth_roi

    # -- forward -----------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, mode=None, image_lr=None, image_hr=None, crops_image_hr=None, depth_gt=None, crop_depths=None,
                bboxs=None, tile_cfg=None, cai_mode="m1", process_num=4, select_patch=-1, shard=None,
                return_device=False, gather_dst=None, next_image_lr=None, frame_index=None, frame_seeds=None, return_uncertainty=False,
                **kwargs):
        """``shard=(rank, world)``: this process computes its share of the frame's tiles (``shard_layout``) and the predictions
        are exchanged (RCCL): all-gather when ``gather_dst`` is None (every rank blends and returns the map), gather to rank
        ``gather_dst`` otherwise (only that rank blends; the others return ``depth=None``).
        ``next_image_lr``: the low-resolution image of the frame the caller will submit NEXT (a video / dataset loop knows
        it): its coarse forward -- one image through the backbone, ~10 ms of kernels that cover a fraction of the chip -- is
        enqueued on a stream of its own beside this frame's tile batches and picked up by the next call (same tensor object);
        results are bit-identical with and without.  In the patch-sharded mode ONE rank computes it (the owner rotates with the frame) and
        broadcasts pyramid + tap tables (``_prefetch_coarse_sharded``); ``frame_index``: the frame's number when the caller's loop is not the
        only one driving this model (tools that emulate several ranks with one object) -- by default the sharded frames are counted.
        B frames per call (image_lr [B,3,h,w], image_hr [B,3,H,W]): depth [B,1,H,W], coarse_prediction [B,1,ph,pw], frame f bit-identical
        to a call on frame f alone; ``frame_seeds`` (B ints): ``random.seed(frame_seeds[f])`` right before frame f's tile plan;
        ``next_image_lr`` may be the next batch.  Not combined with the patch-sharded mode.
        ``return_uncertainty``: the log dict gains ``uncertainty`` -- per pixel, the weighted standard deviation (metres) of the overlapping
        tile predictions around the blended depth -- and ``count_map`` -- the number of tiles covering the pixel (float32, an exact
        integer), both [B,1,H,W] at the depth's resolution, on the host or the device as the depth.  The depth itself is bit-identical to a
        call without it.  Not combined with the patch-sharded mode."""
        if mode != "infer":
            raise NotImplementedError("only mode='infer' is built (training is out of scope, SURVEY.md 2 #12-13)")
        if select_patch != -1:
            raise NotImplementedError("select_patch (feature visualisation hook) is not on the inference path")
        if not (image_lr.is_cuda and image_hr.is_cuda):
            raise RuntimeError("image_lr / image_hr must be on the GPU (tester.py:43-49 moves them); no CPU path")
        n_frames = image_hr.shape[0]
        if image_lr.shape[0] != n_frames:
            raise ValueError(f"image_lr holds {image_lr.shape[0]} frames, image_hr {n_frames}: one low-resolution image per frame")
        if n_frames > 1 and shard is not None and shard[1] > 1:
            raise ValueError(f"{n_frames} frames per call with shard={tuple(shard)}: the patch-sharded mode takes one frame per call")
        if frame_seeds is not None and len(frame_seeds) != n_frames:
            raise ValueError(f"frame_seeds has {len(frame_seeds)} entries for {n_frames} frames")
        stats = bool(return_uncertainty)
        if stats and shard is not None and shard[1] > 1:
            raise ValueError(f"return_uncertainty with shard={tuple(shard)}: the patch-sharded mode does not keep the overlap statistics")
        # every kernel is enqueued on the current device's stream: make the inputs' device current for the whole frame
        with torch.cuda.device(image_hr.device):
            self._next_lr = next_image_lr
            self._frame_index = frame_index
            self._frame_seeds = frame_seeds
            try:
                # (the guard follows the fusion model's own flag: PRV2_F16F6=1 switches the layers on under arith 'bf16x3' as well)
                f16f6 = getattr(self, "arith", None) == "f16f6" or bool(getattr(getattr(self, "refiner_fusion_model", None), "f16f6", False))
                guard = f16f6 and ops.F6Range.active(image_hr.device)
                rnd = random.getstate() if guard else None
                out = self._infer(image_lr, image_hr, depth_gt, tile_cfg, cai_mode, process_num, shard, return_device, gather_dst, stats)
                if guard:
                    # fp16 range guard of the fp16 + fp6 layers (ops.F6Range): a frame in which a layer's input left fp16's range is
                    # computed again with that layer's power-of-two input scale moved (the tile plan's random draws are replayed)
                    reduce = None
                    if shard is not None and shard[1] > 1:  # one decision for all ranks of a patch-sharded frame: the tables' maximum (1 KB all-reduce)
                        import torch.distributed as dist
                        if dist.is_available() and dist.is_initialized():  # (not in the one-process emulations of the ranks: tests' ShardEmulation, tools/shard_model.py)
                            reduce = lambda t: dist.all_reduce(t, op=dist.ReduceOp.MAX)  # noqa: E731
                    self.f6_guarded_frames = getattr(self, "f6_guarded_frames", 0) + 1
                    for attempt in range(3):
                        redo = ops.F6Range.check(image_hr.device, reduce)
                        if ops.F6Range.moved:  # (also an early move without a redo: a captured frame carries the old scales as kernel arguments)
                            self.__dict__.pop("_graphs", None)
                        if not redo:
                            break
                        if attempt == 2:
                            raise RuntimeError(f"f16f6: input range of {len(redo)} layer(s) not representable after two recalibrations "
                                               f"(largest |x x_scale| seen: {[m for _, m, _ in redo]}); use prec='bf16x3'")
                        self.f6_recalibrations = getattr(self, "f6_recalibrations", 0) + 1
                        self.__dict__.pop("_graphs", None)  # (a captured frame carries the old scales)
                        random.setstate(rnd)
                        out = self._infer(image_lr, image_hr, depth_gt, tile_cfg, cai_mode, process_num, shard, return_device, gather_dst, stats)
                return out
            finally:
                self._next_lr = None
                self._frame_index = None
                self._frame_seeds = None

    __call__ = forward

    def _infer(self, image_lr, image_hr, depth_gt, tile_cfg, cai_mode, process_num, shard, return_device, gather_dst, stats=False):
        """The host side of a call of B >= 1 frames: the B tile plans drawn in frame order, ONE frame-major tile list (frame f's tiles are
        rows [f n, (f + 1) n), in the reference's order) whose launch batches may span frames, the coarse forward on the B images, and the
        blend pass by pass for all frames (``_device_frame``).  The plan's coordinates: int32 [(frame, h, w) of every tile | (h, w)
        blend origins], flat; boxes fp32 [B n, 5] = (frame, x1, y1, x2, y2).  ONE frame keeps the single-frame kernels' formats: int32
        [my tiles (h, w) | every tile's blend origin (h, w)] as [n_mine + n, 2] and boxes [n_mine, 4]."""
        tile_cfg = self.tile_cfg if tile_cfg is None else self.prepare_tile_cfg(tile_cfg["image_raw_shape"],
                                                                              tile_cfg["patch_split_num"])
        B = image_hr.shape[0]
        # ---- host: the frames' tile plans (consume Python's ``random`` in the reference's order) ----------------------
        plans = self.plan_frames(tile_cfg, cai_mode, process_num, B, self.__dict__.get("_frame_seeds"))
        self.last_plans = plans
        self.last_plan = plans[-1]
        if shard is not None and shard[1] > 1:
            return self._infer_sharded(image_lr, image_hr, depth_gt, plans[0], tile_cfg, process_num, shard, return_device, gather_dst)
        kinds, counts = [p["kind"] for p in plans[0]], [len(p["raw"]) for p in plans[0]]
        n = sum(counts)
        raw = [[t for p in ps for t in p["raw"]] for ps in plans]
        proc = [t for ps in plans for p in ps for t in p["proc"]]
        if B == 1:
            mine = raw[0] if shard is None else raw[0][shard[0]::shard[1]]  # (shard=(r, 1): the strided debug form)
            n_mine = len(mine)
            tiles_i = torch.tensor(mine + proc, dtype=torch.int32).view(-1, 2)
            boxes_f = torch.from_numpy(self._boxes(mine, tile_cfg)) if self.needs_coarse else torch.zeros((n_mine, 4))
        else:
            n_mine = B * n
            crop = [(f, h, w) for f in range(B) for h, w in raw[f]]
            tiles_i = torch.cat([torch.tensor(crop, dtype=torch.int32).view(-1), torch.tensor(proc, dtype=torch.int32).view(-1)])
            if self.needs_coarse:
                boxes_f = torch.from_numpy(np.concatenate([np.concatenate([np.full((n, 1), f, dtype=np.float32), self._boxes(raw[f], tile_cfg)], 1)
                                                           for f in range(B)]))
            else:
                boxes_f = torch.zeros((n_mine, 5))
        plan = dict(kinds=kinds, counts=counts, n_mine=n_mine, n_all=n, frames=B)
        # (the strided debug form shard=(r, 1) of ONE frame runs eagerly)
        use_graph = bool(getattr(self, "hip_graph", False)) and (shard is None or B > 1) and not ops.PROFILER.enabled
        if use_graph:
            depth, coarse_prediction, extra = self._graph_frame(image_lr, image_hr, tiles_i, boxes_f, plan, tile_cfg, process_num, cai_mode, stats)
        else:
            depth, coarse_prediction, extra = self._eager_frame(image_lr, image_hr, tiles_i, boxes_f, plan, tile_cfg, process_num, stats)
        return self._frame_out(image_lr, depth_gt, depth, coarse_prediction, extra, return_device, use_graph)

    def _eager_frame(self, image_lr, image_hr, tiles_i, boxes_f, plan, tile_cfg, process_num, stats=False):
        """``_device_frame`` on the host plan: its coordinates copied to the device behind whatever the stream is doing"""
        dev = image_hr.device
        return self._device_frame(image_lr, image_hr, tiles_i.to(dev, non_blocking=True), boxes_f.to(dev, non_blocking=True), plan, tile_cfg,
                                  process_num, stats)

    def _frame_out(self, image_lr, depth_gt, depth, coarse_prediction, extra, return_device, use_graph=False):
        """(depth, log) of a frame that has a depth, where the caller wants them (``_out``)"""
        depth = self._out(depth, return_device, use_graph)
        log = dict(rgb=image_lr, depth_pred=depth, depth_gt=depth_gt, coarse_prediction=coarse_prediction)
        if extra is not None:
            log.update(self._stats_out(extra, return_device, use_graph))
        return depth, log

    def _out(self, t, return_device, use_graph):
        """a result where the caller wants it: a pinned host copy, or the device tensor (a captured graph's static outputs are cloned: the
        graph's own output buffer is rewritten by the next replay)"""
        if not return_device:
            return self._to_host(t)
        return t.clone() if use_graph else t

    def _stats_out(self, extra, return_device, use_graph):
        """the overlap statistics (uncertainty, count_map) [B,1,H,W] where the depth goes (``_out``)"""
        unc, count = extra
        return dict(uncertainty=self._out(unc, return_device, use_graph), count_map=self._out(count, return_device, use_graph))

    @staticmethod
    def _to_host(depth):
        """the reference returns a fresh CPU tensor; through torch's caching pinned-memory allocator the 33 MB D2H runs at
        PCIe rate instead of being staged through a pageable buffer (3.4 -> ~1 ms per 4K frame)"""
        hostd = torch.empty(depth.shape, dtype=depth.dtype, pin_memory=True)
        hostd.copy_(depth, non_blocking=True)
        torch.cuda.current_stream(depth.device).synchronize()
        return hostd

    # ==============================================================================================================
    # patch-sharded mode: tiles of ONE frame over the ranks, one process per GPU, RCCL over xGMI
    # ==============================================================================================================
    def _infer_sharded(self, image_lr, image_hr, depth_gt, passes, tile_cfg, process_num, shard, return_device, gather_dst):
        """The frame's plan as ONE int32 tensor [2 * n_all, 2] = (every tile's crop origin | every tile's blend origin), moved to
        the device and overwritten there by rank 0's (an RCCL broadcast enqueued on the stream: no pickling, no host blocking --
        a rank whose ``random`` state differs would otherwise blend the others' predictions at its own coordinates).  Everything
        that depends on coordinates (crops, ROI boxes, blend) reads the device copy; everything the host needs (pass kinds and
        counts, who owns which tile) follows from (cai_mode, process_num, patch_split_num) alone."""
        dev = image_hr.device
        n_all = sum(len(p["raw"]) for p in passes)
        # staged through a pinned buffer (one per plan size, reused once the previous frame's copy out of it has completed): the
        # H2D copy is then really asynchronous -- a pageable source would block the host against the worker streams
        pins = self.__dict__.setdefault("_plan_pins", {})
        ent = pins.get((n_all, str(dev)))
        if ent is None:
            ent = pins[(n_all, str(dev))] = dict(buf=torch.empty((2 * n_all, 2), dtype=torch.int32).pin_memory(), done=None)
        if ent["done"] is not None:
            ent["done"].synchronize()
        ent["buf"].copy_(torch.tensor([t for p in passes for t in p["raw"]] + [t for p in passes for t in p["proc"]], dtype=torch.int32).view(2 * n_all, 2))
        plan_t = ent["buf"].to(dev, non_blocking=True)
        ent["done"] = torch.cuda.Event()
        ent["done"].record(torch.cuda.current_stream(dev))
        plan_t = self._sync_plan_tensor(plan_t)
        plan = dict(kinds=[p["kind"] for p in passes], counts=[len(p["raw"]) for p in passes], n_all=n_all)
        depth, coarse_prediction = self._device_frame_sharded(image_lr, image_hr, plan_t, plan, tile_cfg, shard, gather_dst, process_num)
        if depth is None:  # gather-to-one: this rank's part of the frame is done
            return None, dict(rgb=image_lr, depth_pred=None, depth_gt=depth_gt, coarse_prediction=coarse_prediction)
        return self._frame_out(image_lr, depth_gt, depth, coarse_prediction, None, return_device)

    @staticmethod
    def _sync_plan_tensor(plan_t):
        """rank 0's tile coordinates on every rank (in place; device tensors over RCCL, CPU tensors over gloo in the tests)"""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.broadcast(plan_t, src=0)
        return plan_t

    def _boxes_dev(self, tiles_dev, tile_cfg):
        """``_boxes`` on the device from int32 tile origins [k, 2] (h, w): int -> float32 is exact and the one multiplication by
        the float32 factor is the same IEEE operation, so the boxes equal the host version bit for bit (tested)."""
        H, W = tile_cfg["image_raw_shape"]
        rh, rw = tile_cfg["patch_raw_shape"]
        ph, pw = self.patch_process_shape
        fac = torch.tensor([1 / W * pw, 1 / H * ph, 1 / W * pw, 1 / H * ph], dtype=torch.float32, device=tiles_dev.device)
        h, w = tiles_dev[:, 0], tiles_dev[:, 1]
        bb = torch.stack([w, h, w + rw, h + rh], dim=1).to(torch.float32)
        return bb * fac[None]

    SHARD_DST_COST = 1.5  # what the blending rank does BEHIND the last group (receive, blend, D2H of the map: ~3-4 ms at 4K),
    #                       in tile-times: tiles of the last group move from it to other ranks while that shortens the modelled
    #                       critical path max(others' tiles, its tiles + cost); config key shard_dst_cost

    SHARD_MERGE_BELOW = 8   # from 8 ranks on, a first gather group with fewer than this many tiles PER RANK is merged with the random tiles:
    #                         6 + 4 tiles per rank in two batches under-fill the chip (2.9 ms per tile against 2.2 at 41: the r04 one-GPU model lost
    #                         36 % at 8 ranks to it); one 10-tile batch per rank and one exchange instead -- rank 0 then blends everything behind the
    #                         last batch (order unchanged: bit-identical).  Config key shard_merge_below (0: never merge).

    SHARD_OWNER_COST = 3.5  # what the rank that computes the NEXT frame's coarse pyramid does beside its tiles (the coarse forward: ~8 of the ~11 ms
    #                         every rank used to spend per frame on the headline; the ~2-3 ms of tap tables stay with every rank), in tile-times;
    #                         config key shard_owner_cost

    def shard_layout(self, kinds, counts, world, dst=None, owner=None):
        """Who computes which tile, and what is exchanged when (pure host arithmetic on the plan's pass structure; cached).
        Passes form GATHER GROUPS -- [init + half-offset grids] and [random tiles] -- so that the receiving rank pastes /
        blends the first group (at the re-ensemble resolution) while every rank still computes the second.  Inside a group the
        tiles are dealt round-robin over the ranks; in the LAST group the blending rank ``dst`` hands tiles to the others while
        that shortens max(others' tiles, its tiles + shard_dst_cost) -- its receive + blend + D2H tail.  ``owner``: the rank that computes the
        next frame's coarse pyramid beside this frame's tiles (``_prefetch_coarse_sharded``): it hands tiles over the same way (shard_owner_cost).
        Returns a list of groups: dict(passes=[pass indices], base, n, per, owner=[rank per tile], mine=[[tile offsets in the
        group] per rank], perm=[position of every tile of the group in the rank-major [world * per] gathered stack])."""
        merge_below = int(getattr(self, "shard_merge_below", self.SHARD_MERGE_BELOW))
        key = (tuple(kinds), tuple(counts), int(world), dst, float(getattr(self, "shard_dst_cost", self.SHARD_DST_COST)), merge_below, owner,
               float(getattr(self, "shard_owner_cost", self.SHARD_OWNER_COST)))
        cache = self.__dict__.setdefault("_shard_layouts", {})
        if key in cache:
            return cache[key]
        cost = key[4]
        extra = [0.0] * world  # tile-times a rank spends beside its tiles
        if dst is not None and world > 1:
            extra[dst] += cost
        if owner is not None and world > 1:
            extra[owner] += key[7]
        fixed = [i for i, k in enumerate(kinds) if k != "random"]
        rnd = [i for i, k in enumerate(kinds) if k == "random" and counts[i] > 0]
        groups = []
        id_groups = [ids for ids in (fixed, rnd) if ids]
        if len(id_groups) == 2 and world >= 8 and sum(counts[i] for i in fixed) < merge_below * world:
            id_groups = [sorted(fixed + rnd)]      # one batch and one exchange per rank (pass order kept: the blend walks g["passes"] in order)
        for ids in id_groups:
            n = sum(counts[i] for i in ids)
            share = [n // world] * world
            order = [r for r in range(world - 1, -1, -1) if r != dst] + ([dst] if dst is not None else [])
            for r in order[:n % world]:         # the remainder: highest ranks first, the blending rank last
                share[r] += 1
            if world > 1 and ids is id_groups[-1] and any(extra):
                while True:                     # the busiest of the ranks with side work hands a tile to the least loaded rank while the critical path shrinks
                    busy = [q for q in range(world) if extra[q] > 0 and share[q] > 0]
                    if not busy:
                        break
                    b = max(busy, key=lambda q: (share[q] + extra[q], -q))
                    r = min((q for q in range(world) if q != b), key=lambda q: (share[q] + extra[q], q))
                    now = max(share[q] + extra[q] for q in range(world))
                    then = max(share[q] + extra[q] + (q == r) - (q == b) for q in range(world))
                    if then >= now:
                        break
                    share[b] -= 1
                    share[r] += 1
            owner, left, r = [], list(share), 0
            for _ in range(n):                  # round-robin deal, skipping ranks that are full
                while left[r % world] == 0:
                    r += 1
                owner.append(r % world)
                left[r % world] -= 1
                r += 1
            mine = [[i for i, o in enumerate(owner) if o == q] for q in range(world)]
            per = max(share)
            slot = {}
            for q in range(world):
                for sl, i in enumerate(mine[q]):
                    slot[i] = q * per + sl
            groups.append(dict(passes=ids, base=sum(counts[:ids[0]]), n=n, per=per, owner=owner, mine=mine, share=share,
                               perm=[slot[i] for i in range(n)]))
        cache[key] = groups
        return groups

    def _device_frame_sharded(self, image_lr, image_hr, plan_t, plan, tile_cfg, shard, gather_dst, process_num=4):
        """A frame on rank ``shard[0]`` of ``shard[1]``: coarse forward (every rank; next frame's beside the tiles when
        announced), this rank's tiles group by group (``shard_layout``), the group's prediction stacks exchanged ASYNCHRONOUSLY
        (RCCL gather to ``gather_dst`` / all-gather on the collective's own stream) while the next group computes, and on the
        receiving rank(s) the overlap blend of a group as soon as its stacks have arrived -- in the reference's order, so the
        map is bit-identical to the unsharded one.  No host synchronisation inside."""
        rank, world = shard
        dev = image_hr.device
        ph, pw = self.patch_process_shape
        RH, RW = tile_cfg["patch_reensemble_shape"]
        n_all = plan["n_all"]
        # The NEXT frame's coarse pyramid is computed by ONE rank beside this frame's tiles and broadcast (~100 MB): the owner rotates with the
        # frame index, every other rank spends that time on tiles (shard_layout hands the owner's tiles over).  Every rank replicating the coarse
        # forward was the cap of the patch-sharded mode: ~11 ms beside ~18 ms of tiles at 8 ranks.
        fi = self.__dict__.get("_frame_index")
        if fi is None:
            fi = self._shard_frames = getattr(self, "_shard_frames", -1) + 1  # (every rank calls the frames in the same order)
        next_lr = getattr(self, "_next_lr", None)
        rotate = bool(getattr(self, "shard_rotate_coarse", True)) and self.needs_coarse and next_lr is not None and world > 1 and not ops.PROFILER.enabled
        owner = (fi + 1) % world if rotate and self._coarse_recipe_of(next_lr, tile_cfg) is not None else None
        self.last_coarse_owner = owner
        groups = self.shard_layout(plan["kinds"], plan["counts"], world, gather_dst, owner)
        self.last_shard_layout = groups
        coarse_feats, coarse_prediction, coarse_depth, bs, main, streams = self._frame_setup(image_lr, dev, tile_cfg, process_num)
        image_chw = image_hr[0].contiguous().float()
        raw_all, proc_all = plan_t[:n_all], plan_t[n_all:]

        def layout_dev(g):
            """this rank's tile indices and the group's permutation as device tensors, made once per layout (the layout is cached:
            no per-frame blocking H2D copies)"""
            ent = g.setdefault("_dev", {}).get((rank, str(dev)))
            if ent is None:
                ent = g["_dev"][(rank, str(dev))] = (torch.tensor([g["base"] + i for i in g["mine"][rank]], dtype=torch.int64, device=dev),
                                                     torch.tensor(g["perm"], dtype=torch.int64, device=dev))
            return ent

        # per group: the (padded) stack this rank sends and its tiles' coordinates, allocated before the worker streams start
        stacks, coords = [], []
        for g in groups:
            # (one send stack per layout and rank, zeroed once: rows behind this rank's share are padding nobody reads; the previous frame's
            #  exchange of it was waited for on the main stream before that frame returned, and the worker streams start behind ``ready``)
            sk = g.setdefault("_stacks", {})
            if (rank, str(dev), ph, pw) not in sk:
                sk[(rank, str(dev), ph, pw)] = torch.zeros((g["per"], 1, ph, pw), device=dev)
            stacks.append(sk[(rank, str(dev), ph, pw)])
            idx = layout_dev(g)[0]
            t = raw_all.index_select(0, idx)
            coords.append((t, self._boxes_dev(t, tile_cfg) if self.needs_coarse else None))
        if len(streams) > 1:
            ready = torch.cuda.Event()
            ready.record(main)
            for st in streams:
                st.wait_event(ready)
        receiver = gather_dst is None or rank == gather_dst
        ram = DeviceRunningAverageMap(RH, RW, dev) if receiver else None
        self.last_exchange_bytes = 0
        bi = 0  # batches launched so far: the round-robin over the streams runs on across the groups

        def blend(gi, allp):
            g = groups[gi]
            preds = allp.view(world * g["per"], ph, pw).index_select(0, layout_dev(g)[1])
            self._blend_passes(ram, self._group_passes(plan, groups, gi), preds, proc_all[g["base"]:g["base"] + g["n"]], tile_cfg)

        pending = None  # (group index, exchange handle) whose stacks are on their way
        unwaited = []   # handles of exchanges this rank has not waited for (sending-only ranks): EVERY one is waited for before returning

        def settle():
            """the pending group: blended on the main stream by a receiving rank, kept to be waited for by a sending one"""
            nonlocal receiver
            if not receiver:
                unwaited.append(pending[1])
                return
            allp = pending[1]()
            receiver = allp is not None    # (None on a receiving rank: the tests' recording pass of the shard emulation)
            if receiver:
                blend(pending[0], allp)

        for gi in range(len(groups)):
            t, boxes = coords[gi]
            used = self._run_tiles(image_chw, t, boxes, stacks[gi], bs, streams, bi, (coarse_feats, coarse_depth), tile_cfg)
            bi += len(used)
            if gi == 0:
                if owner is None:
                    self._prefetch_coarse(next_lr, main, tile_cfg, record_recipe=rotate)
                else:
                    self._prefetch_coarse_sharded(next_lr, main, tile_cfg, rank, world, owner)
            if pending is not None:
                settle()                           # (a receiving rank blends the previous group while this one computes)
            for st in used:
                if st is not main:
                    main.wait_stream(st)
            pending = (gi, self._exchange_begin(stacks[gi], shard, gather_dst, gi))
        if pending is not None:
            settle()
        for h in unwaited:  # the send buffers (``stacks``) must outlive their collectives: the main stream waits for each of them
            h()
        if not receiver:
            return None, coarse_prediction
        return ram.avg[None, None], coarse_prediction

    def _exchange_begin(self, mine, shard, dst, group=0):
        """start the exchange of equally sized stacks; returns a callable that makes the current stream wait for it and gives
        the rank-major [world * per, ...] result (None on ranks that do not receive).  RCCL: asynchronous on the collective's
        stream.  A patched ``_exchange`` (tests: single-GPU emulation of the ranks) is called synchronously."""
        self.last_exchange_bytes = getattr(self, "last_exchange_bytes", 0) + mine.numel() * 4 * (shard[1] - 1)
        if "_exchange" in self.__dict__:
            res = self._exchange(mine, shard, dst, group)
            return lambda: res
        import torch.distributed as dist
        rank, world = shard
        if dst is None:
            allp = torch.empty((world * mine.shape[0],) + tuple(mine.shape[1:]), device=mine.device)
            work = dist.all_gather_into_tensor(allp, mine, async_op=True)
            parts = None
        else:
            # (one rank-major receive buffer, its per-rank views as the gather list: no torch.cat behind the collective)
            allp = torch.empty((world * mine.shape[0],) + tuple(mine.shape[1:]), device=mine.device) if rank == dst else None
            parts = list(allp.split(mine.shape[0], dim=0)) if allp is not None else None
            work = dist.gather(mine, parts, dst=dst, async_op=True)

        def result():
            work.wait()  # (RCCL: the current stream waits; gloo: the host does)
            return allp
        return result

    def _boxes_prenorm(self, tiles, tile_cfg) -> np.ndarray:
        """the DATASET's pre-normalised bboxs (pre_norm_bbox=True, u4k_dataset.py:171-176: int64 tensor / W * pw in float32) --
        what the reference's ``mode='train'`` forward receives; differs from the infer path's ``bboxs.int() * (1 / W * pw)``
        (``_boxes``) in the last bit"""
        H, W = (np.float32(v) for v in tile_cfg["image_raw_shape"])
        rh, rw = tile_cfg["patch_raw_shape"]
        ph, pw = (np.float32(v) for v in self.patch_process_shape)
        f = np.float32
        return np.array([[f(w) / W * pw, f(h) / H * ph, f(w + rw) / W * pw, f(h + rh) / H * ph] for h, w in tiles], dtype=np.float32)

    @torch.no_grad()
    def predict_tiles(self, image_lr, image_hr, tiles, tile_cfg=None, prenorm_bbox=False):
        """Per-tile predictions [K, 1, ph, pw] (device) for explicit tile origins ``tiles`` = [(h_start, w_start), ...] of
        patch_raw_shape-sized crops, no blending: what the reference's ``mode='train'`` forward computes for given crops /
        bboxs (coarse forward + ROI of the crop + refiner; patchrefinerplus.py:405-467) -- the building block of
        Tester.run_consistency (tester.py:211-321).  ``prenorm_bbox``: ROI boxes in the dataset's arithmetic (``_boxes_prenorm``)
        instead of the infer path's."""
        if not hasattr(self, "infer_forward") or (not self.needs_coarse and getattr(self, "target", "fine") == "coarse"):
            raise NotImplementedError(f"{type(self).__name__}(target='coarse') has no per-tile path (one backbone forward on image_lr, "
                                      "baseline_pretrain.py:409-411): predict_tiles / run_consistency need a tiling model")
        tile_cfg = self.tile_cfg if tile_cfg is None else self.prepare_tile_cfg(tile_cfg["image_raw_shape"], tile_cfg["patch_split_num"])
        dev = image_hr.device
        ph, pw = self.patch_process_shape
        with torch.cuda.device(dev):
            if self.needs_coarse:
                feats, cp = self.coarse_forward(image_lr)
                self._prepare_frame(feats, tile_cfg)
                cd = Feat(cp.view(1, cp.shape[-2], cp.shape[-1], 1))
            else:
                feats = cd = None
            t_dev = torch.tensor(list(tiles), dtype=torch.int32).view(-1, 2).to(dev)
            mk = self._boxes_prenorm if prenorm_bbox else self._boxes
            boxes = torch.from_numpy(mk(list(tiles), tile_cfg)).to(dev) if self.needs_coarse else None
            preds = torch.empty((len(tiles), 1, ph, pw), device=dev)
            bs = max(1, int(getattr(self, "max_batch", None) or 4))
            self._run_tiles(image_hr[0].contiguous().float(), t_dev, boxes, preds, bs, [torch.cuda.current_stream(dev)], 0, (feats, cd), tile_cfg)
            ops.F6Range.clear(dev)  # (no guarded frame here: what these launches saw must not be judged by the next frame's check)
        return preds

    def _frame_setup(self, image_lr, dev, tile_cfg, process_num, frames=1):
        """what the drivers of a frame start from: this frame's coarse pyramid and its prediction as a ``Feat`` of ``frames`` maps (None
        without ``needs_coarse``), the tile batch size, the main stream and the streams the tile batches go round
        -> (coarse_feats, coarse_prediction, coarse_depth, bs, main, streams)"""
        if self.needs_coarse:
            coarse_feats, coarse_prediction = self._coarse_of(image_lr, tile_cfg)
            coarse_depth = Feat(coarse_prediction.view(frames, coarse_prediction.shape[-2], coarse_prediction.shape[-1], 1))
        else:
            coarse_feats = coarse_prediction = coarse_depth = None
        bs = max(1, int(getattr(self, "max_batch", None) or process_num))
        # Tile batches are independent: they are issued round-robin on ``n_streams`` HIP streams so that the
        # HBM-bound kernels of one batch (gathers, LayerNorm, gate 1x1s) run beside the MFMA-bound convs of another.
        n_streams = max(1, int(getattr(self, "n_streams", None) or 1))
        main = torch.cuda.current_stream(dev)
        return coarse_feats, coarse_prediction, coarse_depth, bs, main, [main] if n_streams == 1 else self._streams(dev, n_streams)

    def _run_tiles(self, image, tiles, boxes, out, bs, streams, bi, coarse, tile_cfg, ready=None):
        """the per-patch networks over a tile list (any batching: per-tile results do not depend on it), ``bs`` tiles per batch, the
        predictions into ``out`` [k, 1, ph, pw] in tile order.  ``bi``: the batches launched before this list -- batch number b (counted
        on from there) goes to streams[b % len(streams)].  ``ready``: an event the first use of every stream waits for (None: the caller
        has made the streams wait).  ``boxes`` None: no coarse ROIs; ``coarse``: (pyramid, depth ``Feat``).  -> the stream of every batch
        launched, in order."""
        used = []
        for s in range(0, tiles.shape[0], bs):
            e = min(s + bs, tiles.shape[0])
            st = streams[bi % len(streams)]
            with torch.cuda.stream(st):
                if ready is not None and bi < len(streams):
                    st.wait_event(ready)
                crops, rois, depth_roi = self._prepare_batch(image, tiles[s:e], boxes[s:e] if boxes is not None else None, tile_cfg, *coarse)
                self.infer_forward(crops, rois, depth_roi, out=out[s:e])
            bi += 1
            used.append(st)
        return used

    def _blend_passes(self, ram, passes, preds, proc, tile_cfg):
        """The overlap blend of ``passes`` = [(kind, k)] into the running-average map ``ram``, in the reference's order: 'init' pastes,
        'grid' updates, 'random' resizes the map to ``image_raw_shape`` and then -- iff the pass has tiles -- updates at ``patch_raw_shape``
        with the mask + 1e-3.  An r-mode whose N // process_num is 0 is a random pass with k = 0: the resize still happens.
        preds [..., n, ph, pw] / proc int32 [..., n, 2]: the predictions and blend origins of exactly these passes' n = sum(k) tiles, in
        pass order; the tile axis is the first of a [H, W] map and the second (behind the frames) of a [B, H, W] one."""
        ph, pw = self.patch_process_shape
        rh, rw = tile_cfg["patch_raw_shape"]
        mask = blend_mask((ph, pw), self.blend_border, 0.0, preds.device)
        o = 0
        for kind, k in passes:
            pr, tdev = preds.narrow(-3, o, k), proc.narrow(-2, o, k)
            o += k
            if kind == "init":
                ram.paste(pr, mask, tdev, ph, pw)
            elif kind == "grid":
                ram.update(pr, mask, tdev, ph, pw)
            else:
                mask_r = blend_mask((rh, rw), self.blend_border, 1e-3, preds.device)  # generatemask(...) + 1e-3 (patchrefinerplus.py:514)
                ram.resize(tile_cfg["image_raw_shape"])
                if k:
                    ram.update(pr, mask_r, tdev, rh, rw)

    @staticmethod
    def _group_passes(plan, groups, gi):
        """[(kind, k)] a receiving rank blends when gather group ``gi`` has arrived: the group's passes, and behind the LAST group the
        passes ``shard_layout`` put into no group because they have no tile to compute -- the empty random pass"""
        ids = list(groups[gi]["passes"])
        if gi == len(groups) - 1:
            ids += range(ids[-1] + 1, len(plan["kinds"]))
        return [(plan["kinds"][i], plan["counts"][i]) for i in ids]

    def _device_frame(self, image_lr, image_hr, tiles_dev, boxes_dev, plan, tile_cfg, process_num, stats=False):
        """Everything of a frame that runs on the device, given the plan's coordinates in device memory: coarse forward, the
        per-patch networks over this rank's tiles (batches round-robin over the HIP streams), the overlap blend -- pass by pass, one
        launch per pass step for all frames.  No host synchronisation inside (captured into a hipGraph by ``_graph_frame``).
        tiles_dev: int32 [n_mine + n_all, 2]: this rank's tile origins, then every tile's blend coordinates.
        B frames (plan["frames"]): tiles_dev flat int32 [(frame, h, w) x B n | (h, w) x B n] frame-major, boxes_dev [B n, 5]; n_all = n.
        -> (depth, coarse_prediction, (uncertainty, count_map) with ``stats``, else None)"""
        dev = image_hr.device
        ph, pw = self.patch_process_shape
        RH, RW = tile_cfg["patch_reensemble_shape"]
        n_mine, n_all = plan["n_mine"], plan["n_all"]
        B = plan["frames"]
        coarse_feats, coarse_prediction, coarse_depth, bs, main, streams = self._frame_setup(image_lr, dev, tile_cfg, process_num, B)
        if B > 1:  # (frame-major: tile batches may span frames)
            tiles_dev, proc_dev = tiles_dev[:3 * n_mine].view(n_mine, 3), tiles_dev[3 * n_mine:].view(B, n_all, 2)
        else:
            proc_dev = tiles_dev[n_mine:]

        # ---- per-patch networks over the tile list (any batching; optional rank sharding) ----
        image_chw = image_hr[0].contiguous().float() if B == 1 else image_hr.contiguous().float()
        preds = torch.empty((n_mine, 1, ph, pw), device=dev)  # this rank's predictions, in tile order
        ready = None
        if len(streams) > 1:
            ready = torch.cuda.Event()
            ready.record(main)
        self._run_tiles(image_chw, tiles_dev[:n_mine], boxes_dev, preds, bs, streams, 0, (coarse_feats, coarse_depth), tile_cfg, ready)
        self._prefetch_coarse(getattr(self, "_next_lr", None), main, tile_cfg)
        if len(streams) > 1:
            for st in streams:
                main.wait_stream(st)

        # ---- overlap blend, in the reference's order: a [H, W] map for one frame, B maps [B, H, W] (preds [B, n, ph, pw], proc int32
        #      [B, n, 2]: frame-major; within a frame the reference's order) otherwise ----
        ram = DeviceRunningAverageMap(RH, RW, dev, frames=None if B == 1 else B, stats=stats)
        preds = preds.view(n_all, ph, pw) if B == 1 else preds.view(B, n_all, ph, pw)
        self._blend_passes(ram, list(zip(plan["kinds"], plan["counts"])), preds, proc_dev, tile_cfg)
        lead = (None, None) if B == 1 else (slice(None), None)  # -> [B, 1, H, W]
        return ram.avg[lead], coarse_prediction, tuple(t[lead] for t in ram.stats_maps()) if stats else None

    def _graph_frame(self, image_lr, image_hr, tiles_i, boxes_f, plan, tile_cfg, process_num, cai_mode, stats=False):
        """``hip_graph=True``: the device side of a frame (``_device_frame``: a few thousand launches on up to ``n_streams``
        streams) is captured once per (mode, geometry, batching) into a hipGraph and replayed per frame; the per-frame inputs
        -- the two images and the plan's coordinates (random tiles change from frame to frame) -- are copied into the graph's
        static buffers first.  The first frame of a key runs eagerly (it fills the constant caches: blend masks, position
        embeddings / relative-position biases), the second is captured.  Results are bit-identical to the eager path."""
        dev = image_hr.device
        key = (cai_mode, process_num, tuple(tile_cfg["image_raw_shape"]), tuple(tile_cfg["patch_split_num"]), tuple(image_lr.shape),
               getattr(self, "max_batch", None), getattr(self, "n_streams", 1), tuple(plan["counts"]), str(dev), bool(stats))
        cache = self.__dict__.setdefault("_graphs", {})
        ent = cache.get(key)
        if ent is None:  # first frame: eager (warm-up of every constant cache)
            cache[key] = "warm"
            return self._eager_frame(image_lr, image_hr, tiles_i, boxes_f, plan, tile_cfg, process_num, stats)
        if ent == "warm":
            st = dict(lr=torch.empty_like(image_lr), hr=torch.empty_like(image_hr), tiles=torch.empty(tiles_i.shape, dtype=torch.int32, device=dev),
                      boxes=torch.empty(boxes_f.shape, dtype=torch.float32, device=dev),
                      h_tiles=torch.empty(tiles_i.shape, dtype=torch.int32).pin_memory(), h_boxes=torch.empty(boxes_f.shape, dtype=torch.float32).pin_memory())
            torch.cuda.current_stream(dev).synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                st["depth"], st["coarse"], st["stats"] = self._device_frame(st["lr"], st["hr"], st["tiles"], st["boxes"], plan, tile_cfg,
                                                                            process_num, stats=stats)
            st["graph"] = g
            cache[key] = ent = st
        if ent.get("staged") is not None:
            ent["staged"].synchronize()  # the previous replay's H2D copies out of the pinned buffers rewritten below
        ent["h_tiles"].copy_(tiles_i)
        ent["h_boxes"].copy_(boxes_f)
        ent["lr"].copy_(image_lr, non_blocking=True)
        ent["hr"].copy_(image_hr, non_blocking=True)
        ent["tiles"].copy_(ent["h_tiles"], non_blocking=True)
        ent["boxes"].copy_(ent["h_boxes"], non_blocking=True)
        ent["staged"] = torch.cuda.Event()
        ent["staged"].record(torch.cuda.current_stream(dev))
        ent["graph"].replay()
        return ent["depth"], (ent["coarse"].clone() if ent["coarse"] is not None else None), ent["stats"]

    def _exchange(self, mine, shard, dst, group=0):
        """blocking form of ``_exchange_begin`` (all-gather when dst is None, gather-to-dst otherwise) -> rank-major
        [world * per, ...] or None.  The single-GPU shard emulation of the tests replaces it on the instance."""
        self.__dict__.setdefault("last_exchange_bytes", 0)
        return self._exchange_begin(mine, shard, dst, group)()

    # -- coarse forward of the NEXT frame beside this frame's tile batches (forward(next_image_lr=...)) -----------------------
    def _prepare_frame(self, coarse_feats, tile_cfg):
        """per-frame work of the per-patch networks that depends on the coarse pyramid only: the coarse half of the fusion convs that
        read cat([., coarse_roi]) (fusion._EncDec.prepare_frame: FusionUnet's encoder_layers_1, BiDirectionalFusion's fusion_layers_1
        and GatedConvUnits) -> the device tensors it created"""
        fm = getattr(self, "refiner_fusion_model", None)
        if fm is None or not hasattr(fm, "prepare_frame"):
            return []
        (rh, rw), (H, W) = tile_cfg["patch_raw_shape"], tile_cfg["image_raw_shape"]
        c_feat = coarse_feats[-self.fusion_feat_level:][::-1]
        fm.prepare_frame(c_feat, (rh / H, rw / W))
        return fm.frame_tensors(c_feat)

    def _coarse_of(self, image_lr, tile_cfg=None):
        """this frame's coarse pyramid: the one prefetched by the previous call if it was made for this very tensor OBJECT,
        unmodified since (the prefetch entry holds the tensor itself: that keeps it alive while the side stream reads it, and
        an address the caching allocator hands out again for another image can never match)"""
        pf = self.__dict__.pop("_coarse_prefetched", None)
        if pf is not None and pf["lr"] is image_lr and pf["version"] == image_lr._version:
            torch.cuda.current_stream(image_lr.device).wait_event(pf["done"])
            for t in pf["tensors"]:  # allocated on the prefetch stream, consumed on this frame's streams from here on
                t.record_stream(torch.cuda.current_stream(image_lr.device))
            self._coarse_hold = pf  # (alive until the next frame replaces it: every consumer stream is long done by then)
            if tile_cfg is not None:
                self._prepare_frame(pf["feats"], tile_cfg)  # (a no-op when the prefetch prepared it for this tiling)
            return pf["feats"], pf["pred"]
        feats, pred = self.coarse_forward(image_lr)
        if tile_cfg is not None:
            self._prepare_frame(feats, tile_cfg)
        return feats, pred

    # -- the next frame's coarse pyramid in the patch-sharded mode: one owner computes, everybody else receives ---------------------
    def _coarse_recipe_key(self, lr, tile_cfg):
        return (tuple(lr.shape), str(lr.device), tuple(tile_cfg["image_raw_shape"]), tuple(tile_cfg["patch_raw_shape"])) if tile_cfg is not None else None

    def _coarse_recipe_of(self, lr, tile_cfg):
        return self.__dict__.get("_coarse_recipes", {}).get(self._coarse_recipe_key(lr, tile_cfg))

    def _record_coarse_recipe(self, lr, tile_cfg, feats, pred):
        """what a rank has to allocate to RECEIVE a coarse pyramid of this image size instead of computing it: the pyramid's buffers and the
        prediction.  (NOT the per-level tap tables ``prepare_frame`` derives from them: 3.8 GB per frame on the headline -- 9 x cout columns at coarse
        resolution + the 3H x 3W knot grids -- against ~100 MB of pyramid; every rank derives its own, ~2 ms.)"""
        bufs, index, fl = [], {}, []
        for f in feats:
            k = f.buf.data_ptr()
            if k not in index:
                index[k] = len(bufs)
                bufs.append(tuple(f.buf.shape))
            fl.append(dict(buf=index[k], c=f.c, c0=f.c0, x2=f.x2))
        self.__dict__.setdefault("_coarse_recipes", {})[self._coarse_recipe_key(lr, tile_cfg)] = dict(bufs=bufs, feats=fl, pred=tuple(pred.shape))

    def _bcast(self, tensors, src):
        """the owner's coarse tensors to every rank, on the CURRENT stream, over a process group of its own (on the frame's communicator the
        broadcast -- which waits for the owner's coarse forward -- would hold up the tile stacks' gathers queued behind it)"""
        if "_bcast_hook" in self.__dict__:  # (tests / tools: one-GPU emulation of the ranks)
            return self._bcast_hook(tensors, src)
        import torch.distributed as dist
        grp = self.__dict__.get("_bcast_group")
        if grp is None:
            grp = self._bcast_group = dist.new_group(ranks=list(range(dist.get_world_size())))
        for t in tensors:
            dist.broadcast(t, src=src, group=grp)

    def _prefetch_coarse_sharded(self, next_lr, main, tile_cfg, rank, world, owner):
        """``_prefetch_coarse`` where only ``owner`` runs the coarse forward: the others allocate the recipe's tensors and receive the pyramid; the
        per-level tap tables are derived from it on every rank.  The pyramid is the owner's bits on every rank: identical to what each rank would
        have computed itself (same kernels, same inputs, one device type)."""
        if torch.cuda.is_current_stream_capturing():
            return
        dev = next_lr.device
        st = self.__dict__.setdefault("_coarse_stream", {}).get(str(dev))
        if st is None:
            st = self._coarse_stream[str(dev)] = torch.cuda.Stream(device=dev, priority=0)
        st.wait_stream(main)
        rec = self._coarse_recipe_of(next_lr, tile_cfg)
        with torch.cuda.stream(st):
            if rank == owner:
                feats, pred = self.coarse_forward(next_lr)
            else:
                bufs = [torch.empty(shape, device=dev, dtype=torch.float32) for shape in rec["bufs"]]
                feats = [Feat(bufs[fr["buf"]], fr["c"], fr["c0"], fr["x2"]) for fr in rec["feats"]]
                pred = torch.empty(rec["pred"], device=dev, dtype=torch.float32)
            uniq, seen = [], set()
            for f in feats:
                if f.buf.data_ptr() not in seen:
                    seen.add(f.buf.data_ptr())
                    uniq.append(f.buf)
            uniq.append(pred)
            self.last_coarse_bcast_bytes = sum(t.numel() * 4 for t in uniq)
            self._bcast(uniq, owner)
            extra = self._prepare_frame(feats, tile_cfg)  # (every rank: the tap tables of the pyramid it now holds)
            uniq = uniq + list(extra)
            done = torch.cuda.Event()
            done.record(st)
        self._coarse_prefetched = dict(lr=next_lr, version=next_lr._version, feats=feats, pred=pred, done=done, tensors=uniq)

    def _prefetch_coarse(self, next_lr, main, tile_cfg=None, record_recipe=False):
        if next_lr is None or not self.needs_coarse or ops.PROFILER.enabled or torch.cuda.is_current_stream_capturing():
            return
        dev = next_lr.device
        st = self.__dict__.setdefault("_coarse_stream", {}).get(str(dev))
        if st is None:
            st = self._coarse_stream[str(dev)] = torch.cuda.Stream(device=dev, priority=0)
        st.wait_stream(main)  # (the image may have been produced on the caller's stream)
        with torch.cuda.stream(st):
            feats, pred = self.coarse_forward(next_lr)
            extra = self._prepare_frame(feats, tile_cfg) if tile_cfg is not None else []
            done = torch.cuda.Event()
            done.record(st)
        tensors = [f.buf for f in feats] + [pred] + list(extra)
        self._coarse_prefetched = dict(lr=next_lr, version=next_lr._version, feats=feats, pred=pred, done=done, tensors=tensors)
        if record_recipe and tile_cfg is not None:  # (patch-sharded mode: from the next frame of this size on, one owner computes and the others receive)
            self._record_coarse_recipe(next_lr, tile_cfg, feats, pred)

    def _invalidate_frame_caches(self):
        """whatever was derived from the weights that have just been replaced: the next frame's prefetched coarse pyramid and
        the captured hipGraphs (they hold raw pointers to the packed weights, relative-position biases and blend masks)"""
        for k in ("_coarse_prefetched", "_coarse_hold", "_graphs"):
            self.__dict__.pop(k, None)

    def _streams(self, dev, n):
        cache = self.__dict__.setdefault("_stream_cache", {})
        if (str(dev), n) not in cache:
            cache[(str(dev), n)] = [torch.cuda.Stream(device=dev) for _ in range(n)]
        return cache[(str(dev), n)]
