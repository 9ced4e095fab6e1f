"""``torch.ops.prv2.*``: the hot path's operators as PyTorch-ROCm custom ops (TORCH_LIBRARY(prv2), csrc/torch_ops.cpp).

This is the operator surface BASELINE.json's north star names ("surfaced to Python as PyTorch-ROCm custom ops"): every op
takes / returns ``at::Tensor``, runs on torch's current HIP stream, allocates through the caching allocator, raises
RuntimeError through TORCH_CHECK, and sits directly on the C ABI of include/prv2.h (libprv2_hip.so).  Registered for the
CUDA (= HIP) dispatch key only: a CPU tensor is rejected by the dispatcher -- there is no CPU implementation to fall into.

    from patchrefinerv2_amd import torch_ops; torch_ops.load()
    y = torch.ops.prv2.conv2d(x_nhwc, w_packed, bias, cout, 3, 3, pad=1, act=torch_ops.ACT_GELU, prec=torch_ops.PREC_BF16X3)

Activations are NHWC float32; a channel slice of a wider NHWC buffer (``buf[..., c0:c0 + c]``) is a valid input and a valid
``out=``, which is how the reference's ``torch.cat`` calls are written in place.
"""
from __future__ import annotations

import os

from .lib import (ABI_VERSION, ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_SOFTPLUS, PREC_BF16, PREC_BF16X3,  # noqa: F401
                  PREC_F32)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libprv2_torch.so")
OPS = ("abi_version", "pack_conv_weight", "conv2d", "conv3x3_ups", "pack_gate_weight", "conv3x3_ln_gate", "layernorm", "attention_fwd", "crop_resize_bilinear", "roi_gather_pyramid", "roi_align",
       "upsample_bilinear_ac", "blend_init", "blend_update", "blend_resize", "zoe_attractor", "zoe_bins_head", "nchw_to_nhwc",
       "nhwc_to_nchw",
       # round 4: every remaining entry point a frame uses (the host mirror's default route can be torch.ops: ops.DISPATCH)
       "conv3x3_tail", "conv3x3_pre", "coarse_tap_knots", "coarse_tap_gather", "conv_cout1", "dwconv2d", "global_avgpool", "se_gate", "channel_scale_",
       "patchify", "assemble_tokens", "split_ss", "layernorm_ss", "gemm_ss", "attention_ss", "bicubic_resize", "depth_pair_fill", "conv_border_bias_",
       "add_nhwc", "zero_pad_channels_", "pack_attention_bias", "upconv3x3",
       # round 5: the fused 32-channel full-resolution chains and the 5x5 composite at the source resolution
       "pack_chain32_weight", "chain32_c2f", "chain32_enc", "upconv5x5", "upconv5x5_lines", "upconv5x5_ring_", "pack_conv3x3_f6_weight", "conv3x3_f6", "conv3x3_ln_gate_f6",
       # ABI 20: B frames per call (tiles / boxes name their frame)
       "crop_resize_frames", "roi_align_frames", "coarse_tap_knots_frames", "coarse_tap_gather_frames", "blend_init_frames", "blend_update_frames",
       "blend_resize_frames",
       # overlap statistics (m2 / ntiles beside the blend's avg / cnt)
       "blend_init_stats", "blend_update_stats", "blend_resize_stats",
       # edge-aware evaluation (Canny, distance transform, dilation, boundary statistics of B frames)
       "depth_preprocess", "canny", "edt_sq", "binary_dilate", "boundary_stats",
       # output stage (order statistics, PNG scanlines, bilinear resize of the coarse map)
       "order_stats", "colorize_rows", "quantize16_rows", "pl_uncertainty_rows", "mask_rows", "upsample_bilinear_map",
       # device deflate: zlib streams of scanline buffers
       "deflate_rows",
       # ground-truth evaluation: raw image / disparity decode and the fused scoring sums
       "u8_image", "disp_gt", "depth_metrics",
       # the general dataset's ground-truth decoders and the scoring of a prediction of another resolution
       "gt_decode", "depth_metrics_lowres",
       # ETHDataset: the image stage and the edge area of its metric splits
       "u8_image_resize", "image_edge_region",
       # CityScapesDataset: the ground-truth decode, kornia's Canny on the colour segmentation map, the two pixel sets of its get_metrics
       "cityscapes_gt", "seg_canny", "cityscapes_masks",
       # KittiDataset / ScanNetDataset: the depth PNG's samples through the kb-crop window or Pillow's NEAREST resize
       "depth16_gt",
       # scale-and-shift-invariant evaluation: the fits, the SSI scores and the error sums of the aligned prediction
       "ssi_metrics",
       # boundary F1 evaluation: the occluding-boundary counts of prediction and ground truth per ratio and direction
       "boundary_f1",
       # sparsification curves (AUSE / AURG) of a per-pixel uncertainty
       "sparsify",
       # geometry export: PLY vertex records and surface-normal scanlines
       "pointcloud_pack", "normal_rows",
       # mesh export: the cloud's vertex records and the face records over them
       "mesh_pack",
       # adaptive mesh export: the vertex and face records of a right-triangulated irregular network over the depth map
       "mesh_adaptive_pack",
       # stereo export: the right-eye view as scanlines, and its source-column maps
       "stereo_rows", "stereo_source",
       # temporal stabilisation: frames of a sequence aligned to and blended with the previous output (state tensors updated in place)
       "temporal_step_",
       # the same with the motion stage in front (also returns the motion stats rows and the blocks' vectors)
       "temporal_motion_step_",
       # depth-of-field export: frames re-rendered through a thin lens, as fp32 planes or as scanlines (each with the focus used)
       "bokeh_render", "bokeh_rows",
       # novel-view export: frames seen from a list of camera poses, as source maps or as scanlines
       "view_source", "view_rows",
       # the gate kernels with the coarse-tap gather inside (tables instead of ``pre``)
       "conv3x3_ln_gate_taps", "conv3x3_ln_gate_f6_taps")
_loaded = False


def load():
    """Register the ops (idempotent) or fail loudly: ImportError when the shim has not been built."""
    global _loaded
    import torch
    if _loaded:
        return torch.ops.prv2
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `make -C patchrefinerv2_amd/csrc` "
                          "(python -c 'import __graft_entry__ as g; g.build()'). There is no fallback.")
    torch.ops.load_library(LIB_PATH)
    if torch.ops.prv2.abi_version() != ABI_VERSION:
        raise ImportError(f"libprv2_torch.so sits on C ABI {torch.ops.prv2.abi_version()}, expected {ABI_VERSION}; rebuild")
    _loaded = True
    return torch.ops.prv2
