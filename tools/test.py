#!/usr/bin/env python
"""User inference CLI with the reference's flags (README.md:51-76, docs/user_infer.md:113-130):

  python tools/test.py CONFIG --ckp-path CKP --cai-mode r32 --cfg-option general_dataloader.dataset.rgb_image_dir=DIR \\
      [--save] --work-dir OUT --test-type general [--gray-scale] --image-raw-shape H W --patch-split-num h w

CONFIG is an MMEngine-style python config (``model=dict(type=..., config=dict(...))``, ``_base_`` supported).
Extras: ``--synthetic-weights`` (the reference has not released checkpoints), ``--prec``, ``--process-num``, ``--max-batch``, ``--streams``.
``--frame-batch N``: N frames per model call on one GPU (per rank in a frame-sharded run), outputs split per frame.
``--generate-pl [--count-thr T]``: Tester.generate_pl instead of run -- pseudo labels with per-pixel uncertainty and tile counts.
``--device-output [--output-workers N]``: with ``--save``, the output files' pixels are produced on the GPU and written by a thread pool.
``--device-deflate``: with ``--device-output``, the files' zlib streams are made on the GPU too (same pixels, different file bytes).
``--save-ply`` / ``--save-normals``: with ``--save``, <name>.ply (binary little-endian point cloud of the result map, coloured from the image)
and <name>_normal.png (surface normals); camera from ``--intrinsics FX FY CX CY`` (pixels of the --image-raw-shape grid) or ``--fov DEG``
(horizontal, default 60); ``--ply-stride S``, ``--ply-edge-thr T`` (flying-pixel filter, <= 0 off), ``--ply-depth-range LO HI``.
``--save-mesh``: with ``--save``, <name>_mesh.ply: the same vertices plus a face element, triangles along the pixel grid (same camera and --ply-* options).
``--mesh-tolerance T`` [``--mesh-block B``]: <name>_mesh.ply becomes the adaptive mesh (a right-triangulated irregular network in blocks of
B x B cells, B a power of two in [2, 64], default 32): triangles up to B pixels wide where the surface is flat to within T, pixel-sized ones at
depth edges; its own vertex list; --ply-stride must be 1.
``--save-bokeh``: with ``--save``, <name>_bokeh.png: the frame with a synthetic depth of field (``--bokeh-aperture M``, ``--bokeh-focus Z`` or
``--bokeh-focus-point U V``, ``--bokeh-max-radius PX``; same camera and --ply-depth-range).
``--save-views N``: with ``--save``, <name>_view_000.png ... <name>_view_{N-1:03d}.png: the frame seen from N poses of a closed camera path
(``--view-motion circle|sway|dolly``, ``--view-amplitude M``, ``--view-focus Z``; same camera, --ply-edge-thr and --ply-depth-range).
``--edge-metrics``: frames with ground truth are also scored on their depth edges (boundary metrics, edge_* / noedge_* splits).
``--ssi-metrics``: frames with ground truth are also scored after a least-squares scale and shift (ssi_* and gm keys, every --test-type).
``--boundary-f1``: frames with ground truth also get the scale-invariant boundary F1 (si_boundary_* keys, and coarse_si_boundary_* of the
coarse prediction; every --test-type).
``--uncert-metrics``: with ``--generate-pl``, frames with ground truth get the sparsification scores of the uncertainty map (AUSE / AURG).
``--test-type normal|test_in|test_out``: the config's val / test_in / test_out dataloader (UnrealStereo4kDataset: raw images and
disparities decoded and scored on the GPU; prints a1 ... sq_rel and see.  ETHDataset: photographs resized and raw float32 depth decoded
on the GPU; prints the thirty keys edge_* / noedge_* / plain, split by the image's edge area); ``--test-type cityscapes``: the config's
val_dataloader when it is a CityScapesDataset (configs/_base_/datasets/cityscapes.py: images, 16-bit disparity PNGs, camera files and colour
segmentation maps decoded on the GPU; prints the seventeen keys a1 ... see, EdgeAcc ... acc -- the depth metrics away from class
boundaries and image edges, the boundary metrics on segmentation edges that are ground-truth depth edges); ``--test-type kitti``: the
val_dataloader when it is a KittiDataset (configs/_base_/datasets/kitti.py: 16-bit depth PNGs read through the 352 x 1216 kb-crop on the
GPU; prints the ten keys a1 ... see inside the Garg crop); ``--test-type scannet``: the val_dataloader when it is a ScanNetDataset
(configs/_base_/datasets/scannet.py: 16-bit depth PNGs brought to the image's size by Pillow's NEAREST rule on the GPU; prints the thirty
keys edge_* / noedge_* / plain, split by the widened ground-truth depth edges).  These three classes are built by their
constructors and are no registry entries, so ``normal`` still answers them with "is not built"; ``general`` is the folder of images -- with
``--cfg-option general_dataloader.dataset.gt_dir=DIR general_dataloader.dataset.gt_format=u4k|eth3d|mid|cityscapes`` a folder with the
reference's ground truth (general_dataset.py:75-158), decoded and scored on the GPU (``image_format=u4k|cityscapes|kitti`` selects
read_image's branch, ``gt_shape=[H,W]`` the shape of ETH3D's raw files).
Multi-GPU: ``sh tools/dist_test.sh CONFIG GPUS [arguments]`` (docs/user_infer.md:113-130): one process per GPU over RCCL;
``--shard frames`` (default, the reference's data parallelism) or ``--shard patches`` (tiles of every frame over the ranks).
"""
import argparse
import ast
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from patchrefinerv2_amd import models, weights as W  # noqa: E402,F401
from patchrefinerv2_amd.registry import DATASETS, Config, build_model  # noqa: E402
from patchrefinerv2_amd.tester import RunnerInfo, Tester  # noqa: E402,F401


def parse_opts(opts):
    out = {}
    for o in opts or []:
        k, v = o.split("=", 1)
        try:
            v = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            pass
        out[k] = v
    return out


# --test-type -> the config section whose ``dataset`` is built (the reference's tools/test.py: normal / test_in / test_out / general)
# ``cityscapes`` / ``kitti`` / ``scannet``: the val_dataloader again, for the dataset classes that are built without being registry
# entries (build_dataset)
TEST_TYPES = dict(general="general_dataloader", normal="val_dataloader", test_in="test_in_dataloader", test_out="test_out_dataloader",
                  cityscapes="val_dataloader", kitti="val_dataloader", scannet="val_dataloader")
# test type -> the class it builds by its constructor
CONSTRUCTED = dict(cityscapes="CityScapesDataset", kitti="KittiDataset", scannet="ScanNetDataset")


def dataset_config(cfg, args):
    """the dataset dict ``--test-type`` selects, with the CLI's overrides (exits with a message when it cannot be built)"""
    if args.test_type not in TEST_TYPES:
        raise SystemExit(f"--test-type {args.test_type}: one of {', '.join(TEST_TYPES)}")
    section = TEST_TYPES[args.test_type]
    if section not in cfg or "dataset" not in cfg[section]:
        raise SystemExit(f"--test-type {args.test_type} needs {section}.dataset in the config; {args.config} has none")
    ds_cfg = cfg[section].dataset.to_dict()
    kind = ds_cfg.get("type")
    if args.test_type in CONSTRUCTED:  # every size is the files' own: nothing of the command line goes into the dataset but --ssi-metrics and --boundary-f1
        if kind != CONSTRUCTED[args.test_type]:
            raise SystemExit(f"--test-type {args.test_type} needs {section}.dataset.type = '{CONSTRUCTED[args.test_type]}'; {args.config} has {kind}")
        if getattr(args, "ssi_metrics", False):
            ds_cfg["ssi_metrics"] = True
        if getattr(args, "boundary_f1", False):
            ds_cfg["boundary_f1"] = True
        return ds_cfg
    if kind not in DATASETS:
        route = {v: k for k, v in CONSTRUCTED.items()}.get(kind)
        raise SystemExit(f"--test-type {args.test_type}: dataset type {kind} is not built (built: ImageDataset, UnrealStereo4kDataset; the "
                         "cityscapes, kitti, scannet and eth decoders are not)"
                         + (f" -- a {kind} val_dataloader runs with --test-type {route}" if route else ""))
    if kind == "UnrealStereo4kDataset":
        ds_cfg["image_raw_shape"] = args.image_raw_shape
    elif kind == "ETHDataset":  # the image's size is transform_cfg.input_size_shallow, the ground truth's gt_shape
        pass
    else:
        ds_cfg["image_resolution"] = args.image_raw_shape
        if args.edge_metrics:
            ds_cfg["edge_metrics"] = True
    if getattr(args, "ssi_metrics", False):  # every dataset class takes it
        ds_cfg["ssi_metrics"] = True
    if getattr(args, "boundary_f1", False):  # likewise
        ds_cfg["boundary_f1"] = True
    return ds_cfg


def build_dataset(ds_cfg):
    """the dataset of ``dataset_config``'s dict: a registry entry, or CityScapesDataset / KittiDataset / ScanNetDataset by its constructor"""
    if ds_cfg.get("type") in CONSTRUCTED.values():
        from patchrefinerv2_amd import tester
        return getattr(tester, ds_cfg["type"])(**{k: v for k, v in ds_cfg.items() if k != "type"})
    return DATASETS.build(ds_cfg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--ckp-path", default=None)
    ap.add_argument("--cai-mode", default="m1")
    ap.add_argument("--cfg-option", nargs="+", default=None)
    ap.add_argument("--save", action="store_true")
    ap.add_argument("--work-dir", default="./work_dir/predictions")
    ap.add_argument("--test-type", default="general", help="general: general_dataloader (a folder of images; with dataset.gt_dir and dataset.gt_format = u4k / eth3d / mid / cityscapes "
                    "set by --cfg-option also the reference's ground truth, decoded and scored on the GPU); normal / test_in / test_out: "
                    "val_dataloader / test_in_dataloader / test_out_dataloader (a dataset with ground truth, e.g. UnrealStereo4kDataset); cityscapes: "
                    "val_dataloader when its dataset is a CityScapesDataset (depth and segmentation-edge metrics, seventeen keys); kitti: "
                    "val_dataloader when its dataset is a KittiDataset (kb-crop, Garg crop, ten keys); scannet: val_dataloader when its dataset is "
                    "a ScanNetDataset (edge_* / noedge_* / plain, thirty keys)")
    ap.add_argument("--gray-scale", action="store_true")
    ap.add_argument("--image-raw-shape", nargs=2, type=int, default=[2160, 3840])
    ap.add_argument("--patch-split-num", nargs=2, type=int, default=[4, 4])
    ap.add_argument("--process-num", type=int, default=4)
    ap.add_argument("--prec", default="bf16x3", choices=["f32", "bf16x3", "f16f6"], help="f16f6: bf16x3 with the 256-channel GatedConvUnit convs of the V2 fusion model in fp16 + block-scaled fp6 (what bench.py runs)")
    ap.add_argument("--max-batch", type=int, default=41, help="tiles per launch batch (the result does not depend on it; config key max_batch wins)")
    ap.add_argument("--streams", type=int, default=3, help="HIP streams the tile batches are spread over (config key n_streams wins)")
    ap.add_argument("--synthetic-weights", action="store_true")
    ap.add_argument("--seed", type=int, default=621)
    ap.add_argument("--frame-batch", type=int, default=1, metavar="N", help="N frames per model call (one GPU; the last group may be "
                    "shorter): outputs are split per frame and bit-identical to one frame per call")
    ap.add_argument("--launcher", default="none", choices=["none", "pytorch"],
                    help="pytorch: started by torch.distributed.run (tools/dist_test.sh): one process per GPU, RCCL process group")
    ap.add_argument("--shard", default="frames", choices=["frames", "patches"],
                    help="multi-GPU: frames = frame f on rank f mod N (the reference's dist_test.sh), patches = the tiles of every "
                         "frame sharded over the ranks, gathered to rank 0 over RCCL")
    ap.add_argument("--consistency", type=int, default=0, metavar="OVERLAP",
                    help="Tester.run_consistency (estimator/tester/tester.py:211): seam error over crops overlapping by OVERLAP pixels (reference: 270)")
    ap.add_argument("--benchmark", action="store_true", help="Tester.benchmark (estimator/tester/tester.py:325) instead of run")
    ap.add_argument("--repeat-times", type=int, default=10)
    ap.add_argument("--generate-pl", action="store_true",
                    help="Tester.generate_pl (estimator/tester/tester.py:132) instead of run: with --save, <name>.png, <name>_uint16.png, "
                         "<name>_uncert_uint16.png, <name>_uncert.png and <name>_count_uint16.png per image (frame-sharded over the ranks)")
    ap.add_argument("--count-thr", type=float, default=0.05,
                    help="--generate-pl: pixels covered by fewer than COUNT_THR x (tiles of the plan) tiles get uncertainty 1")
    ap.add_argument("--edge-metrics", action="store_true",
                    help="with ground truth (dataset gt_dir): add the boundary metrics (EdgeAcc, EdgeComp, precision, recall, f1_score, hamming, "
                         "acc) and the edge_* / noedge_* split of every depth metric (metric.py:210-272, scannet_dataset.py:221-243)")
    ap.add_argument("--ssi-metrics", action="store_true",
                    help="with ground truth (any --test-type): add the scale-and-shift-invariant scores ssi_scale, ssi_shift, ssi_l1, ssi_gm, gm, "
                         "ssi_gm_inv and ssi_a1 ... ssi_sq_rel (losses.py:523-544, :600-700: the prediction aligned to the ground truth by a "
                         "least-squares scale and shift), two fused GPU passes per frame")
    ap.add_argument("--boundary-f1", action="store_true",
                    help="with ground truth (any --test-type): add the scale-invariant boundary F1 of Depth Pro -- si_boundary_f1, si_boundary_p, "
                         "si_boundary_r (ratio tests on neighbouring pixels at ten ratios 1.05 .. 1.25, four directions), one fused GPU pass per "
                         "frame; with a model that has a coarse prediction also coarse_si_boundary_* of that map")
    ap.add_argument("--uncert-metrics", action="store_true",
                    help="with --generate-pl and ground truth (any --test-type whose dataset has it): score the uncertainty map against the "
                         "depth error -- ause_abs_rel, aurg_abs_rel, ause_rmse, aurg_rmse (sparsification curves over 20 levels, pixels under "
                         "--count-thr ordered last), on the GPU; needs a result of the ground truth's shape (an r-mode)")
    ap.add_argument("--device-output", action="store_true",
                    help="with --save: produce the PNG scanlines on the GPU and deflate / write them on a pool of threads while the next "
                         "frame computes (patchrefinerv2_amd/output.py); the files are the host route's")
    ap.add_argument("--device-deflate", action="store_true",
                    help="with --device-output: deflate the scanlines on the GPU as well (csrc/deflate.hip): only compressed bytes are copied "
                         "to the host; the files hold the same pixels as --device-output's, their bytes differ (another deflate stream)")
    ap.add_argument("--output-workers", type=int, default=8, metavar="N", help="--device-output: writer threads (at most 16)")
    ap.add_argument("--save-ply", action="store_true",
                    help="with --save: <name>.ply, a binary little-endian point cloud of the result map (float x y z, uchar red green blue per "
                         "kept pixel, row-major; pinhole camera, x right, y down, z forward), made on the GPU with --device-output")
    ap.add_argument("--save-normals", action="store_true", help="with --save: <name>_normal.png, the camera-facing surface normals as 8-bit RGB (n * 0.5 + 0.5)")
    ap.add_argument("--save-mesh", action="store_true",
                    help="with --save: <name>_mesh.ply, the vertices of --save-ply joined into camera-facing triangles along the pixel grid (binary "
                         "little-endian PLY with a face element; no triangle across an edge --ply-edge-thr splits), made on the GPU with --device-output")
    ap.add_argument("--mesh-tolerance", type=float, default=None, metavar="T",
                    help="--save-mesh: write the adaptive mesh instead -- large triangles where the depth at a hypotenuse midpoint is within T "
                         "(relative, along the ray; finite, >= 0) of a flat triangle's, pixel-sized ones at depth edges and holes; its own "
                         "vertex list, no --ply-stride")
    ap.add_argument("--mesh-block", type=int, default=32, metavar="B",
                    help="--mesh-tolerance: the side of the hierarchy's blocks in cells, the largest triangle's legs (a power of two in [2, 64])")
    ap.add_argument("--save-stereo", action="store_true",
                    help="with --save: <name>_right.png (--stereo-layout: _sbs / _anaglyph), the frame seen from a second eye to the right: "
                         "a per-row forward warp of the image by the result map's disparity with a depth test, disocclusions filled from "
                         "the farther side (camera of --intrinsics / --fov, validity of --ply-depth-range, surfaces split by "
                         "--ply-edge-thr); made on the GPU with --device-output")
    ap.add_argument("--stereo-baseline", type=float, default=0.065, metavar="M", help="--save-stereo: the distance between the eyes in metres")
    ap.add_argument("--stereo-convergence", type=float, default=float("inf"), metavar="Z",
                    help="--save-stereo: the depth that keeps its column (nearer pops out, farther recedes); inf: parallel axes")
    ap.add_argument("--stereo-layout", default="right", choices=["right", "sbs", "anaglyph"],
                    help="--save-stereo: right = the view, sbs = left | right (twice the width), anaglyph = red of left, green and blue of right")
    ap.add_argument("--save-bokeh", action="store_true",
                    help="with --save: <name>_bokeh.png, the frame seen through a thin lens (synthetic depth of field): every pixel spreads over "
                         "its circle of confusion fx * aperture / 2 * |1 / Z - 1 / focus| pixels, a defocused background kept off a sharp "
                         "foreground (camera of --intrinsics / --fov, validity of --ply-depth-range); made on the GPU with --device-output, "
                         "by the host specification otherwise (minutes per 4K frame)")
    ap.add_argument("--bokeh-aperture", type=float, default=0.025, metavar="M", help="--save-bokeh: the lens diameter in metres (0.025: 50 mm at f/2)")
    ap.add_argument("--bokeh-focus", type=float, default=None, metavar="Z", help="--save-bokeh: the distance in focus in metres (default: the depth under --bokeh-focus-point)")
    ap.add_argument("--bokeh-focus-point", nargs=2, type=float, default=[0.5, 0.5], metavar=("U", "V"),
                    help="--save-bokeh without --bokeh-focus: focus on the depth at this point of the frame, (0, 0) top left, (1, 1) bottom right")
    ap.add_argument("--bokeh-max-radius", type=float, default=16.0, metavar="PX", help="--save-bokeh: the cap of the circle of confusion in pixels (at most 32)")
    ap.add_argument("--save-views", type=int, default=0, metavar="N",
                    help="with --save: <name>_view_000.png ... <name>_view_{N-1:03d}.png, the frame seen from N (1 to 120) poses of a closed "
                         "camera path: the result map's own mesh rasterised with a depth test, disocclusions filled from the farther side "
                         "(camera of --intrinsics / --fov, validity of --ply-depth-range, surfaces split by --ply-edge-thr); made on the GPU "
                         "with --device-output, by the host specification otherwise (the specification, not a route for 4K frames: minutes each)")
    ap.add_argument("--view-motion", default="circle", choices=["circle", "sway", "dolly"],
                    help="--save-views: the eye's path: circle = around the optical axis, sway = left and right, dolly = forward and back")
    ap.add_argument("--view-amplitude", type=float, default=0.05, metavar="M", help="--save-views: how far the eye moves, in metres")
    ap.add_argument("--view-focus", type=float, default=float("inf"), metavar="Z",
                    help="--save-views: the depth of the point on the optical axis the camera keeps looking at; inf: it only translates")
    ap.add_argument("--temporal-stabilize", action="store_true",
                    help="treat the frames as one video, in dataset order: every result map is aligned to the previous output by a gated "
                         "least-squares scale and shift and blended with it where the image has not changed (patchrefinerv2_amd/temporal.py; "
                         "on the GPU when the model returns device maps); saved files, exports and metrics see the stabilised map.  One process")
    ap.add_argument("--temporal-alpha", type=float, default=0.5, metavar="A", help="--temporal-stabilize: the weight of the previous output in [0, 1)")
    ap.add_argument("--temporal-tau", type=int, default=6, metavar="T", help="--temporal-stabilize: a pixel is static when its luma moved by at most T (0 .. 255)")
    ap.add_argument("--temporal-rho", type=float, default=0.05, metavar="R", help="--temporal-stabilize: the relative depth change that halves the blend weight (> 0)")
    ap.add_argument("--temporal-anchor", type=float, default=0.9, metavar="K",
                    help="--temporal-stabilize: how much of the fitted scale and shift is applied, in [0, 1] (below 1 the sequence leaks back to the model's own scale)")
    ap.add_argument("--temporal-motion", action="store_true",
                    help="--temporal-stabilize: move the previous output by a field of block vectors first (integer block matching of the two "
                         "frames' lumas, 16 x 16 blocks), so that a panning or hand-held camera does not gate the frame out")
    ap.add_argument("--temporal-motion-range", type=int, default=8, metavar="R",
                    help="--temporal-motion: the search range in quarter-resolution pixels, 1 .. 16 (vectors of up to 4R + 3 pixels a component)")
    ap.add_argument("--intrinsics", nargs=4, type=float, default=None, metavar=("FX", "FY", "CX", "CY"),
                    help="--save-ply / --save-normals: the camera in pixels of the --image-raw-shape grid (scaled to the result's shape)")
    ap.add_argument("--fov", type=float, default=None, metavar="DEG",
                    help="--save-ply / --save-normals without --intrinsics: horizontal field of view (default 60): fx = fy = (W / 2) / tan(fov / 2), "
                         "principal point at the centre")
    ap.add_argument("--ply-stride", type=int, default=1, metavar="S", help="--save-ply: keep the pixels with y %% S == 0 and x %% S == 0")
    ap.add_argument("--ply-edge-thr", type=float, default=0.05, metavar="T",
                    help="--save-ply: drop a pixel when a valid 4-neighbour differs by more than T x the nearer depth (flying pixels); <= 0: off")
    ap.add_argument("--ply-depth-range", nargs=2, type=float, default=[0.0, float("inf")], metavar=("LO", "HI"),
                    help="--save-ply / --save-normals: a pixel is valid when its depth is finite and LO < depth < HI")
    ap.add_argument("--benchmark-iters", nargs=2, type=int, default=[20, 50], metavar=("WARMUP", "TOTAL"))
    args = ap.parse_args()
    if args.device_deflate and not args.device_output:
        ap.error("--device-deflate needs --device-output (it deflates the device route's scanlines)")
    if (args.save_ply or args.save_normals or args.save_mesh or args.save_stereo or args.save_bokeh or args.save_views) and not args.save:
        ap.error("--save-ply / --save-normals / --save-mesh / --save-stereo / --save-bokeh / --save-views need --save (they add files to the "
                 "frames it writes)")
    if not 0 <= args.save_views <= 120:
        ap.error(f"--save-views {args.save_views}: 1 to 120 views")
    if not 0.0 <= args.view_amplitude < float("inf"):
        ap.error(f"--view-amplitude {args.view_amplitude}: finite and not below 0")
    if not args.view_focus > 0.0:
        ap.error(f"--view-focus {args.view_focus}: a depth greater than 0 (inf: the camera only translates)")
    if args.bokeh_focus is not None and not (0 < args.bokeh_focus < float("inf")):
        ap.error(f"--bokeh-focus {args.bokeh_focus}: a finite distance greater than 0")
    if not all(0.0 <= c <= 1.0 for c in args.bokeh_focus_point):
        ap.error(f"--bokeh-focus-point {args.bokeh_focus_point}: inside [0, 1] x [0, 1]")
    if not 0.0 <= args.bokeh_max_radius <= 32.0:
        ap.error(f"--bokeh-max-radius {args.bokeh_max_radius}: in [0, 32]")
    if not 0.0 <= args.bokeh_aperture < float("inf"):
        ap.error(f"--bokeh-aperture {args.bokeh_aperture}: finite and not below 0")
    if args.stereo_convergence == 0 or args.stereo_convergence != args.stereo_convergence:
        ap.error(f"--stereo-convergence {args.stereo_convergence}: a depth other than 0")
    if args.ply_stride < 1:
        ap.error(f"--ply-stride {args.ply_stride}: at least 1")
    if args.mesh_tolerance is not None:
        if not args.save_mesh:
            ap.error("--mesh-tolerance needs --save-mesh (it chooses the mesh that file holds)")
        if args.ply_stride > 1:
            ap.error(f"--mesh-tolerance with --ply-stride {args.ply_stride}: the adaptive mesh has no stride")
        if not (math.isfinite(args.mesh_tolerance) and args.mesh_tolerance >= 0):
            ap.error(f"--mesh-tolerance {args.mesh_tolerance}: finite and at least 0")
        if args.mesh_block < 2 or args.mesh_block > 64 or args.mesh_block & (args.mesh_block - 1):
            ap.error(f"--mesh-block {args.mesh_block}: a power of two in [2, 64]")
    if args.intrinsics is not None and args.fov is not None:
        ap.error("--intrinsics and --fov both given: the camera comes from one of them")
    if not 0.0 <= args.temporal_alpha < 1.0:
        ap.error(f"--temporal-alpha {args.temporal_alpha}: in [0, 1)")
    if not 0 <= args.temporal_tau <= 255:
        ap.error(f"--temporal-tau {args.temporal_tau}: an integer in 0 .. 255")
    if not (args.temporal_rho > 0.0 and args.temporal_rho != float("inf")):
        ap.error(f"--temporal-rho {args.temporal_rho}: positive and finite")
    if not 0.0 <= args.temporal_anchor <= 1.0:
        ap.error(f"--temporal-anchor {args.temporal_anchor}: in [0, 1]")
    if not 1 <= args.temporal_motion_range <= 16:
        ap.error(f"--temporal-motion-range {args.temporal_motion_range}: an integer in 1 .. 16")
    if args.temporal_stabilize and args.generate_pl:
        ap.error("--temporal-stabilize with --generate-pl: pseudo labels are per-image")
    if args.temporal_stabilize and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        ap.error("--temporal-stabilize: one process only (the frames of a sequence are stabilised in dataset order)")
    if args.uncert_metrics and not args.generate_pl:
        ap.error("--uncert-metrics needs --generate-pl (it scores the pseudo label's uncertainty)")

    cfg = Config.fromfile(args.config)
    cfg.merge_from_dict(parse_opts(args.cfg_option))
    ds_cfg = dataset_config(cfg, args)
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
    if world > 1:  # estimator/utils/dist.py:31-33 (init_dist(launcher, backend='nccl')); nccl == RCCL on ROCm
        import torch.distributed as dist
        if not dist.is_initialized():
            dist.init_process_group("nccl", device_id=torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0))))

    mcfg = cfg.model.to_dict()
    # PatchRefiner / PatchRefinerPlus take one ``config`` dict, BaselinePretrain keyword arguments (baseline_pretrain.py:45)
    # (PatchRefinerSemi: the options belong to the student it delegates to, patchrefiner_semi.py:208-210)
    tgt = mcfg["model_cfg_student"] if "model_cfg_student" in mcfg else mcfg
    mopts = tgt["config"] if "config" in tgt else tgt
    mopts["prec"] = args.prec
    mopts.setdefault("max_batch", args.max_batch)  # (the reference's process_num only groups the random tiles of a plan)
    mopts.setdefault("n_streams", args.streams)
    model = build_model(mcfg)
    if args.ckp_path:
        sd = torch.load(args.ckp_path, map_location="cpu")
        print(model.load_dict(sd.get("model_state_dict", sd)))
    elif args.synthetic_weights:
        model.load_state_dict(W.synth_state_dict(model.spec(), seed=0), strict=True)
    else:
        raise SystemExit("give --ckp-path or --synthetic-weights")

    dataset = build_dataset(ds_cfg)
    runner = RunnerInfo(rank=rank, world_size=world, save=args.save, gray_scale=args.gray_scale, work_dir=args.work_dir,
                        device_output=args.device_output, output_workers=args.output_workers, device_deflate=args.device_deflate,
                        save_ply=args.save_ply, save_normals=args.save_normals, save_mesh=args.save_mesh, save_stereo=args.save_stereo,
                        stereo_baseline=args.stereo_baseline, stereo_convergence=args.stereo_convergence, stereo_layout=args.stereo_layout,
                        save_bokeh=args.save_bokeh, bokeh_aperture=args.bokeh_aperture, bokeh_focus=args.bokeh_focus,
                        bokeh_focus_point=tuple(args.bokeh_focus_point), bokeh_max_radius=args.bokeh_max_radius,
                        save_views=args.save_views, view_motion=args.view_motion, view_amplitude=args.view_amplitude, view_focus=args.view_focus,
                        intrinsics=args.intrinsics, fov=args.fov, ply_stride=args.ply_stride, mesh_tolerance=args.mesh_tolerance, mesh_block=args.mesh_block,
                        ply_edge_thr=args.ply_edge_thr, ply_depth_range=tuple(args.ply_depth_range),
                        temporal_stabilize=args.temporal_stabilize, temporal_alpha=args.temporal_alpha, temporal_tau=args.temporal_tau,
                        temporal_rho=args.temporal_rho, temporal_anchor=args.temporal_anchor, temporal_motion=args.temporal_motion,
                        temporal_motion_range=args.temporal_motion_range)
    tester = Tester(cfg, runner, dataset, model)
    if args.consistency:
        for r in tester.run_consistency(image_raw_shape=args.image_raw_shape, patch_split_num=args.patch_split_num, overlap=args.consistency):
            print(f"[rank {rank}] {r['name']}: consistency_error {r['consistency_error']:.6f}")
        print(f"[rank {rank}] consistency_error {tester.last_eval.get('consistency_error', float('nan')):.6f}")
        return
    if args.benchmark:
        b = tester.benchmark(cai_mode=args.cai_mode, process_num=args.process_num, image_raw_shape=args.image_raw_shape,
                             patch_split_num=args.patch_split_num, repeat_times=args.repeat_times,
                             num_warmup=args.benchmark_iters[0], total_iters=args.benchmark_iters[1], seed=args.seed)
        print(f"Average fps of {args.repeat_times} evaluations: {b['average_fps']}")
        print(f"The variance of {args.repeat_times} evaluations: {b['fps_variance']}")
        print(f"Model Flops: {b['flops'] / 1e12:.3f} T  Model Parameters: {b['params'] / 1e6:.1f} M")
        return
    if args.generate_pl:
        if args.shard != "frames":
            raise SystemExit("--generate-pl shards frames over the ranks (--shard frames)")
        for r in tester.generate_pl(cai_mode=args.cai_mode, process_num=args.process_num, image_raw_shape=args.image_raw_shape,
                                    patch_split_num=args.patch_split_num, count_thr=args.count_thr, seed=args.seed, frame_batch=args.frame_batch,
                                    uncert_metrics=args.uncert_metrics):
            print(f"[rank {rank}] {r['name']}: pseudo label {r['shape']} mean {r['mean']:.4f} ({r['n_tiles']} tiles)")
            if "uncert_metrics" in r:
                print(f"[rank {rank}] {r['name']}: " + ", ".join(f"{k} {float(v):.6f}" for k, v in r["uncert_metrics"].items()))
        if args.uncert_metrics and getattr(tester, "last_eval", None):  # (this rank's frames: generate_pl does not collect)
            print(f"[rank {rank}] " + ", ".join(f"{k} {v:.4f}" for k, v in tester.last_eval.items()))
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
        return
    results = tester.run(cai_mode=args.cai_mode, process_num=args.process_num, image_raw_shape=args.image_raw_shape,
                         patch_split_num=args.patch_split_num, seed=args.seed, shard=args.shard, frame_batch=args.frame_batch)
    if rank == 0 or world == 1:  # (frame-sharded runs: rank 0 holds every rank's results, collected like collect_results_gpu)
        for r in results:
            print(f"[rank {rank}] {r['name']}: depth {r['shape']} mean {r['mean']:.4f}")
            if "temporal" in r:
                t = r["temporal"]
                print(f"[rank {rank}] {r['name']}: temporal " + ("reset" if t["reset"] else f"scale {t['scale']:.6f} shift {t['shift']:.6f} static "
                      f"{t['static_fraction']:.3f} change {t['change_before']:.6f} -> {t['change_after']:.6f}"))
                if t.get("motion") and t["motion"]["blocks"]:
                    m = t["motion"]
                    print(f"[rank {rank}] {r['name']}: motion (dy, dx) mean ({m['mean_dy']:.2f}, {m['mean_dx']:.2f}), moving "
                          f"{100.0 * m['moving_fraction']:.1f} %, max {m['max_abs']} px, SAD {m['sad_zero']} -> {m['sad']}")
            if args.test_type != "general" and "metrics" in r:  # a dataset evaluation: the frame's own row
                print(f"[rank {rank}] {r['name']}: " + ", ".join(f"{k} {float(v):.6f}" for k, v in r["metrics"].items()))
        if getattr(tester, "last_eval", None):  # frames that came with ground truth (dataset gt_dir, or a dataset with its own)
            print(f"[rank {rank}] " + ", ".join(f"{k} {v:.4f}" for k, v in tester.last_eval.items()))
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
