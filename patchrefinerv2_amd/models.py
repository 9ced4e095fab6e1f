"""The models: what a frame's tiles run through.  How a frame is executed (tiling -> per-patch networks -> overlap blend, all on the
device) is frame.py's ``FrameDriver``, which every tiling model inherits.

Host-side mirrors, registered under the reference ``type`` names:
  BaselinePretrain   estimator/models/baseline_pretrain.py:45-464 (tile planner, regular/random tile)
  PatchRefiner       estimator/models/patchrefiner.py:54-404        (V1: DA2 coarse + DA2 per patch + FusionUnet)
  PatchRefinerPlus   estimator/models/patchrefinerplus.py:60-533    (V2: DA2 coarse + LightWeightRefiner + BiDirectionalFusion)
Call contract (tester.py:69, patchrefinerplus.py:367-380,526-530):
  depth, log = model(mode='infer', cai_mode, process_num, tile_cfg, image_lr, image_hr)
  depth: [1,1,H',W'] fp32 CPU tensor; log['coarse_prediction']: [1,1,ph,pw] device tensor.
  B frames per call: image_lr [B,3,h,w], image_hr [B,3,H,W] -> depth [B,1,H',W'], coarse_prediction [B,1,ph,pw]; frame f is
  bit-identical to a call on frame f alone (the B tile plans are drawn in frame order, ``frame_seeds`` reseeds per frame).
"""
from __future__ import annotations

from typing import List

import numpy as np
import torch

from . import ops
from .dav2 import DepthAnythingV2, IMAGENET_MEAN, IMAGENET_STD, StateDictModule
from .frame import DeviceRunningAverageMap, FrameDriver, blend_mask, generatemask  # noqa: F401  (re-exported: they lived here)
from .fusion import BiDirectionalFusion, BiDirectionalFusionHeavy, FusionUnet
from .ops import Feat
from .refiner import LightWeightRefiner
from .registry import MODELS, ConfigDict, build_model

MODELS.register_module(module=FusionUnet)
MODELS.register_module(module=BiDirectionalFusion)
MODELS.register_module(module=BiDirectionalFusionHeavy)
MODELS.register_module(module=LightWeightRefiner)


@MODELS.register_module()
class SILogLoss:  # training-only; constructed by the reference at model init (patchrefinerplus.py:83)
    def __init__(self, **kw):
        pass


@MODELS.register_module()
class GradMatchLoss:
    def __init__(self, **kw):
        pass


class Resizer:
    """``model.resizer`` of the reference: ResizeDA (external/depth_anything/transform.py:6-129,
    keep_aspect_ratio=False, 'minimal', multiple of 14) or ResizeZoe (midas.py:171-174, fixed 384x512),
    executed by the crop+resize HIP kernel."""

    def __init__(self, width: int, height: int, kind: str = "da"):
        if kind == "da":
            self.out_hw = (int(np.round(height / 14) * 14), int(np.round(width / 14) * 14))
        else:
            self.out_hw = (384, 512)
        self.kind = kind

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("Resizer runs on the GPU (HIP crop+resize kernel); move the image to the device")
        B, _, H, W = x.shape
        oh, ow = self.out_hw
        out = Feat.alloc(B, oh, ow, 3, x.device, pad_to=1)
        zero = torch.zeros((1, 2), dtype=torch.int32, device=x.device)
        for b in range(B):
            ops.crop_resize(x[b].contiguous().float(), zero, H, W, oh, ow, None, None, out.batch(b, b + 1))
        return out.to_nchw()


def _cfg(config):
    if isinstance(config, ConfigDict):
        return config
    if hasattr(config, "to_dict"):
        return ConfigDict(config.to_dict())
    return ConfigDict(dict(config))


class _PatchModel(FrameDriver, StateDictModule):
    """What PatchRefiner / PatchRefinerPlus share (they inherit it from BaselinePretrain in the reference): the tiling + blending
    driver (``FrameDriver``), the checkpoint contract and the coarse branch."""

    crop_channels = 3
    crop_mean, crop_std = IMAGENET_MEAN, IMAGENET_STD
    STRICT_DA_ZOE = False
    supports_return_device = True  # forward(return_device=True): the depth map stays on the GPU (Tester scores it there)
    blend_border = 0.15      # generatemask(..., border=0.15) (patchrefinerplus.py:485); BaselinePretrain: the default 0.1
    needs_coarse = True      # coarse forward + ROI pyramid per tile (False: BaselinePretrain(target='fine'))

    def load_state_dict(self, sd, strict: bool = True):
        res = super().load_state_dict(sd, strict=strict)
        self._invalidate_frame_caches()
        return res

    # -- checkpoint contract (patchrefinerplus.py:212-216) ------------------------------------------
    def load_dict(self, sd):
        """patchrefinerplus.py:212-213 (``load_state_dict(strict=False)``) made checkpoint-ready: key variants of the two
        un-vendored packages (timm's flattened / unflattened feature-net names, a DDP ``module.`` prefix, BatchNorm bookkeeping
        buffers) are rewritten by ``weights.remap_state_dict``; whatever still does not match is REPORTED, grouped by module
        (``weights.diagnose_state_dict``) -- the reference prints the bare key lists -- and a forward with parameters still
        missing raises 'weights not loaded' instead of running on garbage.  The report is kept in ``self.last_load_report``."""
        import warnings
        from . import weights as W_
        spec = self.spec()
        sd, applied = W_.remap_state_dict(sd, spec)
        diag = W_.diagnose_state_dict(spec, sd)  # BEFORE loading: load_state_dict raises on the first shape mismatch
        if diag["shape_mismatch"]:
            raise RuntimeError("load_dict: checkpoint tensors whose shape differs from the model's -- " + W_.format_diagnosis(diag))
        res = self.load_state_dict(sd, strict=False)
        self.last_load_report = dict(diag, remapped=applied)
        if applied:
            warnings.warn("load_dict: renamed checkpoint keys -- " + ", ".join(f"{k}: {v}" for k, v in applied.items()))
        if res["missing_keys"] or res["unexpected_keys"]:
            warnings.warn("load_dict: " + W_.format_diagnosis(diag))
        return res

    def get_save_dict(self):
        return self.state_dict()

    # -- PyTorchModelHubMixin's on-disk layout (patchrefinerplus.py:39,60): <dir>/config.json + <dir>/model.safetensors.
    #    Local directories only: there is no hub access from this build.
    def save_pretrained(self, save_directory):
        import json
        import os
        from safetensors.torch import save_file
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, "config.json"), "w") as f:
            json.dump(self.config.to_dict(), f, indent=2, sort_keys=True)
        save_file({k: v.detach().cpu().contiguous() for k, v in self.get_save_dict().items()},
                  os.path.join(save_directory, "model.safetensors"))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, **config_overrides):
        """``Model.from_pretrained(dir)``: config.json -> ``cls(config)``, model.safetensors -> ``load_dict`` (the mixin
        builds the class with ``config=`` and loads non-strictly, like the reference's own load_dict)."""
        import json
        import os
        from safetensors.torch import load_file
        d = str(pretrained_model_name_or_path)
        if not os.path.isdir(d):
            raise FileNotFoundError(f"from_pretrained: '{d}' is not a local directory (no hub access in this build)")
        with open(os.path.join(d, "config.json")) as f:
            cfg = json.load(f)
        cfg.update(config_overrides)
        m = cls(cfg)
        m.load_dict(load_file(os.path.join(d, "model.safetensors")))
        return m

    def _make_da2(self, branch_cfg, max_depth):
        mc = dict(branch_cfg["model_cfg"])
        m = DepthAnythingV2(**{**mc, "max_depth": max_depth}, device=self.device, prec=self.prec)
        # load_state_dict(torch.load(branch['pretrained'])) -- a bare state dict, strict (patchrefiner.py:94,118)
        self._load_ckpt(m, branch_cfg.get("pretrained"), None, True, "DepthAnythingV2 weights")
        return m

    @staticmethod
    def _load_ckpt(module, path, key, strict, what, keep=None):
        """The constructor-time checkpoint loads of the reference (patchrefiner.py:82-148, patchrefinerplus.py:104-206):
        ``torch.load(path, map_location='cpu')[key]`` into ``module``.  A path that does not exist is skipped with a
        warning (the reference would die in torch.load): the weights then have to arrive through load_state_dict /
        load_dict, and a forward without them raises 'weights not loaded'."""
        if path is None:
            return None
        import os
        import warnings
        if not os.path.exists(str(path)):
            warnings.warn(f"{what}: checkpoint '{path}' does not exist -- skipped; load the weights with load_dict()")
            return None
        sd = torch.load(str(path), map_location="cpu")
        if key is not None:
            sd = sd[key]
        if keep is not None:
            sd = {k: v for k, v in sd.items() if keep(k)}
        widen = getattr(getattr(module, "refiner_fine_branch", None), "coarse_condition", True)  # (:144: only with coarse_condition)
        for k in list(sd):
            # the reference loads a 3-channel timm stem first and then widens it to 4 input channels with a zero
            # plane (stem surgery, patchrefinerplus.py:144-200): same result, done on the checkpoint
            if widen and k.endswith(("refiner_encoder.conv_stem.weight", "refiner_encoder.stem_0.weight")) and sd[k].shape[1] == 3:
                w = torch.zeros((sd[k].shape[0], 4) + tuple(sd[k].shape[2:]), dtype=sd[k].dtype)
                w[:, :3] = sd[k]
                sd[k] = w
        return module.load_state_dict(sd, strict=strict)

    def _common_init(self, config):
        config = _cfg(config)
        self.config = config
        self.min_depth, self.max_depth = config.min_depth, config.max_depth
        self.patch_process_shape = tuple(config.patch_process_shape)
        self.tile_cfg = self.prepare_tile_cfg(config.image_raw_shape, config.patch_split_num)
        self.prec = ops.L.PREC_NAMES[config.get("prec", "f32")]
        self.arith = config.get("prec", "f32")  # the model-level name ("f16f6": bf16x3 + the fp16 / fp6 layers; handed to the fusion model as is)
        self.device = torch.device(config.get("device", "cuda"))
        self.max_batch = config.get("max_batch", None)
        self.n_streams = config.get("n_streams", 1)
        self.hip_graph = bool(config.get("hip_graph", False))  # capture + replay the device side of a frame (_graph_frame)
        self.shard_dst_cost = float(config.get("shard_dst_cost", self.SHARD_DST_COST))  # patch-sharded mode (shard_layout)
        self.shard_owner_cost = float(config.get("shard_owner_cost", self.SHARD_OWNER_COST))
        self.shard_rotate_coarse = bool(config.get("shard_rotate_coarse", True))  # one rotating rank computes the next frame's coarse pyramid
        self.strategy_refiner_target = config.strategy_refiner_target
        self.fusion_feat_level = config.fusion_feat_level
        ctype = config.coarse_branch["type"]
        pcm = config.get("pretrain_coarse_model", None)
        if ctype == "DA2":
            self.coarse_branch = self._make_da2(config.coarse_branch, config.max_depth)
            self.resizer = Resizer(self.patch_process_shape[1], self.patch_process_shape[0], "da")
            self._load_ckpt(self.coarse_branch, pcm, "model_state_dict", True, "pretrain_coarse_model")
        elif ctype in ("DA-ZoeDepth", "ZoeDepth"):
            # ZoeDepth.build(**coarse_branch) (patchrefinerplus.py:102-116): midas_model_type picks the core -- MiDaS
            # DPT_BEiT_L_384 (the default) or a DepthAnything ViT; the config's ``type`` picks the resizer
            from .zoedepth import ZoeDepth
            zc = {k: v for k, v in config.coarse_branch.to_dict().items() if k != "type"}
            self.coarse_branch = ZoeDepth(device=self.device, prec=self.prec, **zc)
            if ctype == "ZoeDepth":
                # ResizeZoe.__call__ is hard-coded to 384 x 512 whatever it is constructed with (midas.py:171-174)
                if tuple(self.patch_process_shape) != (384, 512):
                    raise ValueError(f"coarse_branch type 'ZoeDepth' resizes every image to 384 x 512 (midas.py:171-174): "
                                     f"patch_process_shape {list(self.patch_process_shape)} cannot work (the reference fails too)")
                self.resizer = Resizer(512, 384, "zoe")
            else:
                self.resizer = Resizer(self.patch_process_shape[1], self.patch_process_shape[0], "da")
            # strict only for DA-ZoeDepth under PatchRefinerPlus (patchrefinerplus.py:108,116; patchrefiner.py:82,89)
            self._load_ckpt(self.coarse_branch, pcm, "model_state_dict", ctype == "DA-ZoeDepth" and self.STRICT_DA_ZOE,
                            "pretrain_coarse_model")
        else:
            raise NotImplementedError(f"coarse_branch type {ctype!r}")
        if self.strategy_refiner_target != "offset_coarse":
            raise NotImplementedError("strategy_refiner_target: every shipped config uses 'offset_coarse'")
        return config

    def coarse_forward(self, image_lr):
        """patchrefinerplus.py:218-237: one backbone forward; pyramid low -> high + metric depth."""
        out = self.coarse_branch(image_lr, return_final_centers=True)
        t = out["temp_features"]
        feats = [t["x_d0"], t["x_blocks_feat_0"], t["x_blocks_feat_1"], t["x_blocks_feat_2"], t["x_blocks_feat_3"],
                 t["midas_final_feat"]]
        return feats, out["metric_depth"]


@MODELS.register_module()
class BaselinePretrain(_PatchModel):
    """estimator/models/baseline_pretrain.py:44-93 (constructor: keyword arguments, not one ``config``), 377-464.
    target='coarse': ONE backbone forward on ``image_lr``, no tiling -- returns the DEVICE tensor [1,1,ph,pw] and
    dict(rgb, depth_pred, depth_gt) (:409-411,464).  target='fine': the tiling driver with the bare backbone on every
    tile (``infer_forward`` :144-146), blend mask border 0.1 (generatemask's default, :420,447) and -- unlike the two
    refiners -- N random_tile CALLS for r<N>, i.e. N * process_num random tiles (:449-452); returns (CPU depth, {})."""

    blend_border = 0.1
    needs_coarse = False

    def __init__(self, coarse_branch=None, fine_branch=None, sigloss=None, min_depth=1e-3, max_depth=80,
                 image_raw_shape=(2160, 3840), patch_process_shape=(384, 512), patch_split_num=(4, 4), target="coarse",
                 coarse_branch_zoe=None, device="cuda", prec="f32", max_batch=None, n_streams=1):
        super().__init__()
        self.min_depth, self.max_depth = min_depth, max_depth
        self.patch_process_shape = tuple(patch_process_shape)
        self.tile_cfg = self.prepare_tile_cfg(image_raw_shape, patch_split_num)
        self.prec = ops.L.PREC_NAMES[prec] if isinstance(prec, str) else prec
        self.arith = prec if isinstance(prec, str) else ops.L.PREC_LABEL[prec]
        self.device = torch.device(device)
        self.max_batch, self.n_streams = max_batch, n_streams
        self.target = target
        if target not in ("coarse", "fine"):
            raise NotImplementedError(f"BaselinePretrain target {target!r}")  # baseline_pretrain.py:406,461
        bcfg = _cfg(coarse_branch if target == "coarse" else fine_branch)
        btype = bcfg["type"]
        if btype == "DA2" and target == "coarse":
            branch = self._make_da2(bcfg, max_depth)
        elif btype in ("ZoeDepth", "DA-ZoeDepth"):
            from .zoedepth import ZoeDepth
            branch = ZoeDepth(device=self.device, prec=self.prec, **{k: v for k, v in bcfg.to_dict().items() if k != "type"})
        else:
            raise NotImplementedError(f"BaselinePretrain(target={target!r}) with branch type {btype!r} "
                                      "(baseline_pretrain.py:68-90 builds none either)")
        self.resizer = Resizer(self.patch_process_shape[1], self.patch_process_shape[0], "zoe" if btype == "ZoeDepth" else "da")
        name = "coarse_branch" if target == "coarse" else "fine_branch"
        setattr(self, name, branch)
        self._branch = branch
        self._children = {name: branch}
        self.crop_mean, self.crop_std = getattr(branch, "input_mean", IMAGENET_MEAN), getattr(branch, "input_std", IMAGENET_STD)

    def _pack(self):
        pass

    # baseline_pretrain.py:126-142: checkpoints hold the bare branch
    def load_dict(self, sd):
        self._invalidate_frame_caches()
        return self._branch.load_state_dict(sd, strict=False)

    def get_save_dict(self):
        return self._branch.state_dict()

    def random_calls(self, cai_mode, process_num):
        return int(cai_mode[1:])  # ``for i in range(patch_num)`` (baseline_pretrain.py:449-452)

    @torch.no_grad()
    def forward(self, mode=None, image_lr=None, image_hr=None, depth_gt=None, **kw):
        if mode == "train":
            raise NotImplementedError("only inference is built (training is out of scope, SURVEY.md 2 #12-13)")
        if self.target == "coarse":
            if kw.get("return_uncertainty"):
                raise ValueError("return_uncertainty: BaselinePretrain(target='coarse') predicts the whole frame at once -- no tiles overlap")
            if not image_lr.is_cuda:
                raise RuntimeError("image_lr must be on the GPU (tester.py:43-49 moves it); no CPU path")
            with torch.cuda.device(image_lr.device):
                depth = self.coarse_branch(image_lr)["metric_depth"]
            return depth, dict(rgb=image_lr, depth_pred=depth, depth_gt=depth_gt)
        depth, log = super().forward(mode="infer", image_lr=image_lr, image_hr=image_hr, depth_gt=depth_gt, **kw)
        return depth, {k: log[k] for k in ("uncertainty", "count_map") if k in log}

    __call__ = forward

    def infer_forward(self, crops: Feat, rois, depth_roi, out=None):
        """baseline_pretrain.py:144-146: ``self.fine_branch(imgs_crop)['metric_depth']``"""
        d = self.fine_branch.forward_nhwc(crops)["metric_depth"]
        if out is not None:
            out.copy_(d)
            return out
        return d


@MODELS.register_module()
class PatchRefiner(_PatchModel):
    """V1 (estimator/models/patchrefiner.py:54)."""

    def __init__(self, config):
        super().__init__()
        config = self._common_init(config)
        fb = config.refiner.fine_branch
        if fb["type"] == "DA2":
            self.refiner_fine_branch = self._make_da2(fb, config.max_depth)
        elif fb["type"] in ("ZoeDepth", "DA-ZoeDepth"):  # patchrefiner.py:104-115: ZoeDepth.build(**fine_branch)
            from .zoedepth import ZoeDepth
            self.refiner_fine_branch = ZoeDepth(device=self.device, prec=self.prec,
                                                **{k: v for k, v in fb.to_dict().items() if k != "type"})
            self.crop_mean, self.crop_std = self.refiner_fine_branch.input_mean, self.refiner_fine_branch.input_std
        else:
            raise NotImplementedError(f"refiner fine_branch type {fb['type']!r}")
        self._load_ckpt(self.refiner_fine_branch, config.get("pretrain_fine_model", None), "model_state_dict",
                        fb["type"] == "DA2", "pretrain_fine_model")
        self.refiner_fusion_model = build_model({**config.refiner.fusion_model.to_dict(), "device": self.device,
                                                 "prec": self.arith if self.arith == "f16f6" else self.prec})
        self._children = dict(coarse_branch=self.coarse_branch, refiner_fine_branch=self.refiner_fine_branch,
                              refiner_fusion_model=self.refiner_fusion_model)
        # config.pretrained: the refiner part only unless load_whole (patchrefiner.py:125-143)
        whole = bool(config.get("load_whole", False))
        self._load_ckpt(self, config.get("pretrained", None), "model_state_dict", False, "pretrained",
                        keep=None if whole else (lambda k: "coarse_branch" not in k))

    def _pack(self):
        pass

    def get_save_dict(self):  # patchrefiner.py:158-166: the coarse branch is not saved
        return {k: v for k, v in self.state_dict().items() if "coarse_branch." not in k}

    def infer_forward(self, crops: Feat, rois: List[Feat], depth_roi: Feat, out=None):
        """patchrefiner.py:258-283."""
        fine = self.refiner_fine_branch.forward_nhwc(crops)
        t = fine["temp_features"]
        r_feats = [t["x_d0"], t["x_blocks_feat_0"], t["x_blocks_feat_1"], t["x_blocks_feat_2"], t["x_blocks_feat_3"],
                   t["midas_final_feat"]]
        n = self.fusion_feat_level
        base = depth_roi.buf.view(depth_roi.n, 1, depth_roi.h, depth_roi.w)
        return self.refiner_fusion_model(c_feat=rois[-n:][::-1], f_feat=r_feats[-n:][::-1], pred1=base,
                                         pred2=fine["metric_depth"], update_base=base, out=out)


@MODELS.register_module()
class PatchRefinerSemi(StateDictModule):
    """estimator/models/patchrefiner_semi.py:46-210, the INFERENCE side: the configs the real-domain checkpoints ship with
    (patchrefinerv2_dav2/semi_kitti.py, *_cs_semi_*, pr_ssi_*) name this type; at test time ``forward`` hands everything to the student
    (:198-210).  The teacher, the pseudo-label / edge / distillation machinery and ``mode='train'`` are training and are
    not built: only ``model_cfg_student`` is instantiated.  State-dict names carry the ``student_model.`` prefix as in the reference."""

    def __init__(self, model_cfg_student, teacher_pretrain=None, model_cfg_teacher=None, **_training_only):
        super().__init__()
        self.student_model = build_model(model_cfg_student)
        self._children = dict(student_model=self.student_model)
        self.device, self.prec = self.student_model.device, self.student_model.prec

    def _pack(self):
        pass

    def __getattr__(self, name):  # resizer, tile_cfg, patch_process_shape, min / max_depth, predict_tiles ... are the student's (:163)
        if name in ("student_model", "_children", "_spec", "_sd"):
            raise AttributeError(name)
        return getattr(self.student_model, name)

    def load_dict(self, sd):
        """patchrefiner_semi.py:110-116: old checkpoints hold teacher + student (only the ``student_model.`` keys are loaded here: the
        teacher is not built), new ones only the student's own names (strict=False there too)"""
        if "student_model.coarse_branch.core.core.pretrained.model.cls_token" in sd:
            return self.load_state_dict({k: v for k, v in sd.items() if k.startswith("student_model.")}, strict=True)
        return self.student_model.load_state_dict(sd, strict=False)

    def get_save_dict(self):
        return self.student_model.get_save_dict()

    def forward(self, mode=None, image_lr=None, image_hr=None, depth_gt=None, cai_mode="m1", **kw):
        if mode == "train":
            raise NotImplementedError("PatchRefinerSemi: only inference is built (training is out of scope, SURVEY.md 2 #12-14)")
        # (:208-210 forwards cai_mode but neither tile_cfg nor process_num: the student runs with its configured tiling -- unless the
        #  caller passes them, which the reference's wrapper would have dropped)
        extra = {k: v for k, v in kw.items() if k in ("tile_cfg", "process_num", "next_image_lr", "return_device", "frame_seeds", "return_uncertainty") and v is not None}
        return self.student_model(mode=mode, image_lr=image_lr, image_hr=image_hr, depth_gt=depth_gt, cai_mode=cai_mode, **extra)

    __call__ = forward


@MODELS.register_module()
class PatchRefinerPlus(_PatchModel):
    """V2 (estimator/models/patchrefinerplus.py:60)."""

    crop_channels = 4
    STRICT_DA_ZOE = True

    def __init__(self, config):
        super().__init__()
        config = self._common_init(config)
        if config.get("pretrain_stage", False):
            raise NotImplementedError("pretrain_stage=True is a training configuration")
        self.refiner_fine_branch = build_model({**config.refiner.fine_branch.to_dict(), "device": self.device,
                                                "prec": self.prec})
        self.refiner_fusion_model = build_model({**config.refiner.fusion_model.to_dict(), "device": self.device,
                                                 "prec": self.arith if self.arith == "f16f6" else self.prec})
        self.crop_mean, self.crop_std = self.refiner_fine_branch.mean, self.refiner_fine_branch.std
        self._children = dict(coarse_branch=self.coarse_branch, refiner_fine_branch=self.refiner_fine_branch,
                              refiner_fusion_model=self.refiner_fusion_model)
        # patchrefinerplus.py:132-135 (before the stem surgery: a 3-channel conv_stem checkpoint) and :202-205
        self._load_ckpt(self, config.get("pretrained", None), "model_state_dict", False, "pretrained")
        self._load_ckpt(self, config.get("whole_pretrained", None), "model_state_dict", False, "whole_pretrained")

    def _pack(self):
        pass

    def infer_forward(self, crops: Feat, rois: List[Feat], depth_roi: Feat, out=None):
        """patchrefinerplus.py:330-365: encoder on [norm(rgb), coarse depth roi] then BiDirectionalFusion."""
        ops.upsample_bilinear(depth_roi, crops.h, crops.w, out=crops.slice(3, 1))  # 4th input channel (exact copy)
        f_feat, f_sizes = self.refiner_fine_branch(crops)
        n = self.fusion_feat_level
        base = depth_roi.buf.view(depth_roi.n, 1, depth_roi.h, depth_roi.w)
        zeros = torch.zeros_like(base)  # out_depth = zeros (lightweight_refiner.py:320); replaced by c2f's output
        return self.refiner_fusion_model(c_feat=rois[-n:][::-1], f_feat=f_feat, pred1=base, pred2=zeros,
                                         update_base=base, f_sizes=f_sizes, out=out)
