"""Inference driver (the caller above the hot path); the datasets it walks are in datasets.py, the PNG container in output.py.

Tester.run          estimator/tester/tester.py:52-127 (frame loop, model call contract, uint16 PNG x256)
Tester.generate_pl  estimator/tester/tester.py:132-181 (pseudo labels: depth, uncertainty and tile-count PNGs)
``runner_info.device_output`` (tools/test.py --device-output) routes the saved files through output.OutputStage: scanlines made on
the GPU, deflate on a writer pool; the default is the host route below.  ``runner_info.device_deflate`` (--device-deflate, needs
device_output) makes the zlib streams on the GPU as well: the files hold the device route's pixels, but not its bytes (the deflate
stream differs from zlib's).
``runner_info.save_ply`` / ``save_normals`` (--save-ply / --save-normals, with ``save``) add the frame's geometry: <name>.ply (a
binary point cloud of the result map, coloured from the image) and <name>_normal.png (its surface normals);
``runner_info.save_mesh`` (--save-mesh) adds <name>_mesh.ply (the cloud's vertices joined into triangles; with
``runner_info.mesh_tolerance`` / ``mesh_block`` (--mesh-tolerance T, --mesh-block B) the adaptive mesh instead: large triangles
where the surface is flat, pixel-sized ones at depth edges, its own vertex list) and
``runner_info.save_stereo`` (--save-stereo) <name>_right.png / _sbs.png / _anaglyph.png (the right-eye view),
``runner_info.save_bokeh`` (--save-bokeh) <name>_bokeh.png (the frame with a synthetic depth of field),
``runner_info.save_views`` = N (--save-views N; 0: off) <name>_view_000.png ... (the frame seen from N poses of a closed camera path:
``view_motion``, ``view_amplitude``, ``view_focus``) -- from the device map
with the output stage, from output.py's host specification otherwise; the same files either way.
``runner_info.temporal_stabilize`` (--temporal-stabilize; ``temporal_alpha`` / ``_tau`` / ``_rho`` / ``_anchor``) treats the dataset as
one video: every result map goes through temporal.TemporalStabilizer before it is saved, exported or scored;
``runner_info.temporal_motion`` (--temporal-motion; ``temporal_motion_range`` = R in 1 .. 16) puts its block-motion stage in front, so
that a moving camera does not gate the frames out.
With ``--save``: <name>.png (colour map, tester.py:72-87), <name>_uint16.png (depth x 256, :89-91), <name>_coarse.png
(coarse prediction resized to the raw shape, :93-96) and <name>_edge.png (Canny edges of the log depth, widened by one pixel,
:98-106; metrics.depth_edges) -- colour maps and metrics in metrics.py, PNGs through a dependency-free encoder (output.py).
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

# importing this module registers the datasets, and the six classes stay importable from here (tools/ and the tests do both);
# read_image only because tests/test_host_logic.py imports it from here.  Everything else of datasets.py is imported from there.
from .datasets import (CityScapesDataset, ETHDataset, ImageDataset, KittiDataset, ScanNetDataset, UnrealStereo4kDataset,  # noqa: F401
                       read_image)
from .output import write_png8, write_png16


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
        results = []
        rank, world = self.runner_info.rank, getattr(self.runner_info, "world_size", 1)
        patches = shard == "patches" and world > 1
        if max(1, int(frame_batch)) > 1 and patches:
            raise ValueError("frame_batch > 1 with shard='patches': the patch-sharded mode takes one frame per call")
        stab = self._stabilizer()
        stage = self.last_output_stage = self._output_stage()  # (kept: its bytes_d2h / files counters)
        # with ground truth the frame is scored on the device (metrics.compute_metrics_device): ask for the device map
        for items, hr, result, log in self._frames(stage, cai_mode, process_num, image_raw_shape, patch_split_num, seed, frame_batch,
                                                   device_scoring=True, patches=patches, want_device=stab is not None):
            if result is None:  # patch-sharded: only rank 0 holds the map
                continue
            temporal = None
            if stab is not None:  # the group's frames in dataset order; the coarse prediction is left alone
                result, temporal = stab.step(result, hr)
            coarse = log.get("coarse_prediction")
            for f, item in enumerate(items):
                one = len(items) == 1
                self._emit(results, item, result if one else result[f:f + 1], coarse if one or coarse is None else coarse[f:f + 1],
                           image_raw_shape, stage,
                           **({} if temporal is None else dict(temporal=self._temporal_entry(temporal[f]))))
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
        if stab is not None:  # the flicker of the sequence before / after, over the frames that had a predecessor
            import warnings
            rows = [r["temporal"] for r in results if not r["temporal"]["reset"]]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                means = {"temporal_" + k: float(np.mean([t[k] for t in rows])) if rows else float("nan") for k in ("change_before", "change_after")}
                if stab.motion_range:  # the share of moving blocks, over the frames whose motion stage ran
                    moved = [r["temporal"]["motion"]["moving_fraction"] for r in results if r["temporal"]["motion"]["blocks"]]
                    means["temporal_moving_fraction"] = float(np.mean(moved)) if moved else float("nan")
            scored = bool(results) and "metrics" in results[0]
            self.last_eval = {**(self.last_eval if scored else {}), **means}
        return results

    TEMPORAL_KEYS = ("reset", "static_fraction", "scale", "shift", "change_before", "change_after")  # of a result entry's ``temporal``

    @classmethod
    def _temporal_entry(cls, stats):
        """a result entry's ``temporal`` from the frame's stats dict: ``TEMPORAL_KEYS``, and ``motion`` when the motion stage is on"""
        entry = {k: stats[k] for k in cls.TEMPORAL_KEYS}
        return entry if stats["motion"] is None else dict(entry, motion=stats["motion"])

    def _stabilizer(self):
        """the run's ``temporal.TemporalStabilizer`` when ``runner_info.temporal_stabilize`` is set (``temporal_alpha``, ``temporal_tau``,
        ``temporal_rho``, ``temporal_anchor``: its parameters; ``temporal_motion`` and ``temporal_motion_range``: its motion stage), else
        None.  The frames are one sequence in dataset order: a run over several ranks is rejected (frame sharding breaks the order; the
        patch-sharded mode is not built)."""
        info = self.runner_info
        motion = bool(getattr(info, "temporal_motion", False))
        if not getattr(info, "temporal_stabilize", False):
            if motion:
                raise ValueError("temporal_motion without temporal_stabilize: the motion stage is a part of the temporal stabiliser")
            return None
        if getattr(info, "world_size", 1) > 1:
            raise ValueError("temporal_stabilize: one process only -- the frames of a sequence are stabilised in dataset order, which a "
                             f"run over {info.world_size} ranks does not keep")
        from .temporal import DEFAULTS, TemporalStabilizer
        mrange = getattr(info, "temporal_motion_range", None)
        return TemporalStabilizer(**{k: getattr(info, "temporal_" + k, None) if getattr(info, "temporal_" + k, None) is not None else v
                                     for k, v in DEFAULTS.items()}, motion=motion, motion_range=8 if mrange is None else mrange)

    def _frames(self, stage, cai_mode, process_num, image_raw_shape, patch_split_num, seed, frame_batch, device_scoring, patches=False,
                want_device=False, **model_kw):
        """The frame loop of ``run`` and ``generate_pl`` -> (items, image_hr on the device, result, log) per model call.  Frame f is dealt to rank f mod world
        (``patches``: every frame to every rank, the call sharded over them) and ``frame_batch`` of a rank's frames make one call.  The
        next group is loaded BEFORE the model call, so that its decode and uploads overlap the current frames' tiles, and its
        low-resolution images are announced to a model that runs a coarse forward (``next_image_lr``).  ``seed``: every frame's plan
        from that seed.  The maps stay on the device (``return_device``) for the output stage, and with ``device_scoring`` for a
        group with ground truth -- with ``want_device`` for every group -- when the model can return them there.  ``model_kw`` goes to the
        model as it is."""
        import random
        rank, world = self.runner_info.rank, getattr(self.runner_info, "world_size", 1)
        fb = max(1, int(frame_batch))
        prefetch = bool(getattr(self.model, "needs_coarse", False))
        todo = list(range(len(self.dataloader))) if patches else list(range(rank, len(self.dataloader), world))
        groups = [todo[i:i + fb] for i in range(0, len(todo), fb)]
        device = getattr(self.model, "device", "cuda")

        def load(idxs):
            items = [self.dataloader[idx] for idx in idxs]
            hr = torch.stack([item["image_hr"] for item in items]).to(device)
            return items, hr, self.model.resizer(hr)

        nxt = load(groups[0]) if groups else None
        for n, idxs in enumerate(groups):
            items, hr, lr = nxt
            nxt = load(groups[n + 1]) if n + 1 < len(groups) else None
            kw = dict(model_kw)
            if seed is not None:
                if len(idxs) == 1:  # (one frame: the same plan as frame_seeds=[seed], which reseeds right before it is drawn)
                    random.seed(seed)
                else:  # (every frame's plan from the same seed, as one frame per call does)
                    kw["frame_seeds"] = [seed] * len(idxs)
            scored = device_scoring and any(item.get("depth_gt") is not None for item in items)
            if stage is not None or ((scored or want_device) and getattr(self.model, "supports_return_device", False)):
                kw.update(return_device=True)
            if patches:
                kw.update(shard=(rank, world), gather_dst=0)
            if prefetch and nxt is not None:
                kw["next_image_lr"] = nxt[2]
            tile_cfg = dict(image_raw_shape=list(image_raw_shape), patch_split_num=list(patch_split_num))
            result, log = self.model(mode="infer", cai_mode=cai_mode, process_num=process_num, tile_cfg=tile_cfg,
                                     image_lr=lr, image_hr=hr, **kw)
            yield items, hr, result, log

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

    def _colour(self, pseudo_label=False):
        """-> (cmap, (vminp, vmaxp)) of a frame's colour PNG: every dataset branch of tester.py:76-84 but cityscapes maps to Spectral,
        a pseudo label to magma_r, over the 0..100 percentiles; ``gray_scale``: gray_r (a frame's with colorize's default 2..95)"""
        if getattr(self.runner_info, "gray_scale", False):
            return "gray_r", (0, 100) if pseudo_label else (2, 95)
        cityscapes = getattr(self.dataloader, "dataset_name", "") == "cityscapes"
        return ("magma_r" if pseudo_label or cityscapes else "Spectral"), (0, 100)

    def _geometry(self, result, image_raw_shape):
        """the keyword arguments of ``submit_geometry`` / ``write_geometry_host`` for a result map, None without ``save_ply`` /
        ``save_normals`` / ``save_mesh`` / ``save_stereo``: the camera of ``runner_info.intrinsics`` (fx fy cx cy in pixels of the raw grid) or ``runner_info.fov``
        (degrees, default 60) scaled to the result's grid, ``ply_depth_range``, ``ply_edge_thr``, ``ply_stride``; with ``mesh_tolerance``
        that and ``mesh_block`` (32), checked; with ``save_stereo`` the
        ``stereo`` dict of ``stereo_baseline`` (default 0.065), ``stereo_convergence`` (inf) and ``stereo_layout`` ('right'); with
        ``save_bokeh`` the ``bokeh`` dict of ``bokeh_aperture`` (0.025), ``bokeh_focus`` (None: the depth under ``bokeh_focus_point``,
        default (0.5, 0.5)) and ``bokeh_max_radius`` (16); with ``save_views`` = N > 0 the ``views`` dict of N, ``view_motion`` ('circle'),
        ``view_amplitude`` (0.05) and ``view_focus`` (inf)"""
        info = self.runner_info
        ply, normals, mesh, stereo, bokeh = (bool(getattr(info, k, False)) for k in ("save_ply", "save_normals", "save_mesh", "save_stereo", "save_bokeh"))
        views = int(getattr(info, "save_views", 0) or 0)
        if not (info.save and (ply or normals or mesh or stereo or bokeh or views)):
            return None
        from .output import camera_intrinsics
        k = camera_intrinsics(image_raw_shape, result.shape[-2:], getattr(info, "intrinsics", None), getattr(info, "fov", None) or 60.0)
        tol = getattr(info, "mesh_tolerance", None)
        if tol is not None:  # (the adaptive mesh: <name>_mesh.ply with its own vertex list; it has no stride)
            from .output import mesh_adaptive_arguments
            tol, block = mesh_adaptive_arguments(tol, getattr(info, "mesh_block", 32))
            if not mesh or int(getattr(info, "ply_stride", 1)) != 1:
                raise ValueError("runner_info.mesh_tolerance needs save_mesh and ply_stride 1")
        return dict(intrinsics=k, depth_range=tuple(getattr(info, "ply_depth_range", None) or (0.0, float("inf"))),
                    edge_thr=float(getattr(info, "ply_edge_thr", 0.05)), stride=int(getattr(info, "ply_stride", 1)), ply=ply, normals=normals, mesh=mesh,
                    **(dict(mesh_tolerance=tol, mesh_block=block) if tol is not None else {}),
                    **(dict(stereo=dict(baseline=float(getattr(info, "stereo_baseline", 0.065)),
                                        convergence=float(getattr(info, "stereo_convergence", float("inf"))),
                                        layout=getattr(info, "stereo_layout", "right"))) if stereo else {}),
                    **(dict(bokeh=dict(aperture=float(getattr(info, "bokeh_aperture", 0.025)), focus=getattr(info, "bokeh_focus", None),
                                       focus_point=tuple(getattr(info, "bokeh_focus_point", None) or (0.5, 0.5)),
                                       max_radius=float(getattr(info, "bokeh_max_radius", 16.0)))) if bokeh else {}),
                    **(dict(views=dict(count=views, motion=getattr(info, "view_motion", "circle"), amplitude=float(getattr(info, "view_amplitude", 0.05)),
                                       focus=float(getattr(info, "view_focus", float("inf"))))) if views else {}))

    def _entry(self, item, result, score=None, coarse=None, **extra):
        """one frame's result entry.  ``mean``: a host map's fp32 mean, a device map's float64 sum on the device (equal within that
        sum's rounding).  ``score``: the map the dataset scores when the item carries ground truth.  ``coarse``: the model's coarse
        prediction of the frame; a dataset with ``boundary_f1`` then also gets ``coarse_si_boundary_f1 / _p / _r``: the coarse map's
        boundary scores with the same arguments, sampled to the ground truth's grid inside the kernel (one more call per frame) --
        beside ``si_boundary_*`` they say how much boundary quality the refiner added"""
        mean = result.mean(dtype=torch.float64) if result.is_cuda else result.mean()
        entry = dict(name=item["img_file_basename"], shape=tuple(result.shape), mean=float(mean), **extra)
        if score is not None and item.get("depth_gt") is not None:
            seg = {} if item.get("seg_image") is None else dict(seg_image=item["seg_image"])  # (CityScapesDataset with_seg_map)
            entry["metrics"] = self.dataloader.get_metrics(item["depth_gt"], score, disp_gt_edges=item.get("boundary"),
                                                           image_hr=item["image_hr"], **seg)
            if coarse is not None and getattr(self.dataloader, "boundary_f1", False):
                from .metrics import compute_boundary_f1_fused
                scores = compute_boundary_f1_fused(item["depth_gt"], coarse, fuse_resize=True, **self.dataloader.boundary_args())
                entry["metrics"].update({"coarse_" + k: v for k, v in scores.items()})
        return entry

    def _emit(self, results, item, result, coarse, image_raw_shape, stage=None, **extra):
        """one frame's outputs: PNGs (--save), its metrics and its result entry (``extra``: further keys of the entry).  With ``stage``
        the same files come from scanlines produced on the GPU (the device output stage)"""
        base = os.path.join(self.runner_info.work_dir, item["img_file_basename"])
        cmap, (lo, hi) = self._colour()
        if stage is not None:
            if not result.is_cuda:
                raise ValueError("device_output: the model returned a host map")
            stage.submit_frame(base, result, coarse, image_raw_shape, cmap=cmap, percentiles=(lo, hi))
            geo = self._geometry(result, image_raw_shape)
            if geo is not None:
                stage.submit_geometry(base, result, item["image_hr"], **geo)
            results.append(self._entry(item, result, score=result, coarse=coarse, **extra))
            return
        score = result  # (a device map is scored where it is)
        result = result.cpu()  # BaselinePretrain(target='coarse') hands back the device tensor (baseline_pretrain.py:464)
        if self.runner_info.save:
            from .metrics import colorize, depth_edges
            os.makedirs(self.runner_info.work_dir, exist_ok=True)
            # raw depth as 16-bit PNG, multiplier 256 (tester.py:89-91)
            write_png16(base + "_uint16.png", (result.squeeze().numpy() * 256).astype("uint16"))
            write_png8(base + ".png", np.ascontiguousarray(colorize(result, cmap=cmap, vminp=lo, vmaxp=hi)[:, :, :3]))
            write_png8(base + "_edge.png", depth_edges(result).astype(np.uint8) * 255)  # tester.py:99-106
            if coarse is not None:  # absent for BaselinePretrain
                coarse_map = F.interpolate(coarse.cpu(), tuple(image_raw_shape), mode="bilinear")
                write_png8(base + "_coarse.png", np.ascontiguousarray(colorize(coarse_map, cmap="Spectral", vminp=0, vmaxp=100)[:, :, :3]))
            geo = self._geometry(result, image_raw_shape)
            if geo is not None:  # the host route of the geometry export: the host specification itself
                from .output import write_geometry_host
                image = torch.as_tensor(item["image_hr"]).cpu().float().numpy()
                write_geometry_host(base, result.squeeze().numpy(), image.reshape(3, *image.shape[-2:]), geo.pop("intrinsics"), **geo)
        results.append(self._entry(item, result, score=score, coarse=coarse, **extra))

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
        if getattr(self.runner_info, "temporal_stabilize", False):
            raise ValueError("temporal_stabilize with generate_pl: pseudo labels are per-image (the stabiliser carries one frame into the next)")
        results = []
        stage = self.last_output_stage = self._output_stage()  # (kept: its bytes_d2h / files counters)
        # (with uncert_metrics the maps stay where they are scored)
        for items, _, result, log in self._frames(stage, cai_mode, process_num, image_raw_shape, patch_split_num, seed, frame_batch,
                                                  device_scoring=bool(uncert_metrics), return_uncertainty=True):
            # the plan's tile count (every frame of a call has the same passes; only random positions differ)
            n_tiles = sum(len(p["raw"]) for p in self.model.last_plan)
            for f, item in enumerate(items):
                depth, maps = result[f:f + 1], (log["uncertainty"][f:f + 1], log["count_map"][f:f + 1])
                extra = dict(n_tiles=n_tiles)
                if uncert_metrics and item.get("depth_gt") is not None:
                    extra["uncert_metrics"] = self._uncert_metrics(item, depth, *maps, count_thr * n_tiles, cai_mode)
                if stage is not None:  # the five files from scanlines produced on the GPU
                    stage.submit_pseudo_label(os.path.join(self.runner_info.work_dir, item["img_file_basename"]), depth, *maps, n_tiles,
                                              count_thr, cmap=self._colour(pseudo_label=True)[0])
                else:
                    depth = depth.cpu()
                    if self.runner_info.save:
                        self._write_pl(item["img_file_basename"], depth, *(m.cpu() for m in maps), n_tiles, count_thr)
                results.append(self._entry(item, depth, **extra))
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
        cmap, (lo, hi) = self._colour(pseudo_label=True)
        write_png8(base + ".png", np.ascontiguousarray(colorize(depth, cmap=cmap, vminp=lo, vmaxp=hi)[:, :, :3]))
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
