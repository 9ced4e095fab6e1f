"""CPU: B frames per call (ABI 20) -- the *_frames entry points are declared, bound and exported, reject bad arguments without a
GPU, have torch ops with schemas, and the B-frame tile plan consumes Python's ``random`` exactly like B sequential plans."""
import ctypes
import os
import random
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SYMBOLS = ("prv2_crop_resize_frames", "prv2_roi_align_frames", "prv2_roi_align_x2_frames", "prv2_coarse_tap_knots_frames",
                 "prv2_coarse_tap_gather_frames", "prv2_blend_paste_frames", "prv2_blend_update_frames", "prv2_blend_resize_frames")
FRAME_OPS = ("crop_resize_frames", "roi_align_frames", "coarse_tap_knots_frames", "coarse_tap_gather_frames", "blend_init_frames",
             "blend_update_frames", "blend_resize_frames")


def test_frame_entry_points_declared_bound_and_exported():
    from patchrefinerv2_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert re.search(r"#define PRV2_ABI_VERSION 20\b", hdr) and L.ABI_VERSION == 20
    lib = L.load()
    assert lib.prv2_abi_version() == 20
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in FRAME_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in L.SIGNATURES and hasattr(raw, name), name


def _err(lib):
    return lib.prv2_last_error().decode()


def test_frame_entry_points_reject_bad_arguments_without_gpu():
    from patchrefinerv2_amd import lib as L
    lib = L.load()
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its argument check before a launch
    m3 = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    # null pointers
    assert lib.prv2_crop_resize_frames(None, 2, 64, 64, p, 3, 32, 32, 16, 16, m3, m3, p, 4, None) != 0 and "null" in _err(lib)
    assert lib.prv2_roi_align_frames(p, 2, 8, 8, 4, 4, None, 3, 1.0, 4, 4, p, 4, None) != 0 and "null" in _err(lib)
    assert lib.prv2_coarse_tap_knots_frames(None, 2, 8, 8, 4, 36, 0.25, 0.25, p, 4, None) != 0 and "null" in _err(lib)
    assert lib.prv2_coarse_tap_gather_frames(p, None, 2, 8, 8, 4, 4, 36, 0.25, 0.25, p, 3, 1.0, 4, 4, p, 4, None) != 0 and "null" in _err(lib)
    assert lib.prv2_blend_paste_frames(p, None, 2, 32, 32, p, 8, 8, 256, p, p, 4, 4, 8, 8, None) != 0 and "null" in _err(lib)
    assert lib.prv2_blend_resize_frames(p, p, 2, 8, 8, None, p, 16, 16, None) != 0
    # B < 1
    for b in (0, -1):
        assert lib.prv2_crop_resize_frames(p, b, 64, 64, p, 3, 32, 32, 16, 16, m3, m3, p, 4, None) != 0 and "n_frames" in _err(lib)
        assert lib.prv2_roi_align_frames(p, b, 8, 8, 4, 4, p, 3, 1.0, 4, 4, p, 4, None) != 0 and "n_frames" in _err(lib)
        assert lib.prv2_roi_align_x2_frames(p, b, 8, 8, 8, 8, p, 3, 1.0, 4, 4, p, 8, None) != 0 and "n_frames" in _err(lib)
        assert lib.prv2_coarse_tap_knots_frames(p, b, 8, 8, 4, 36, 0.25, 0.25, p, 4, None) != 0 and "n_frames" in _err(lib)
        assert lib.prv2_coarse_tap_gather_frames(p, p, b, 8, 8, 4, 4, 36, 0.25, 0.25, p, 3, 1.0, 4, 4, p, 4, None) != 0
        assert lib.prv2_blend_paste_frames(p, p, b, 32, 32, p, 8, 8, 256, p, p, 4, 4, 8, 8, None) != 0 and "n_frames" in _err(lib)
        assert lib.prv2_blend_update_frames(p, p, b, 32, 32, p, 8, 8, 256, p, p, 4, 4, 8, 8, None) != 0 and "n_frames" in _err(lib)
        assert lib.prv2_blend_resize_frames(p, p, b, 8, 8, p, p, 16, 16, None) != 0 and "frame count" in _err(lib)
    # too many frames for the grid
    assert lib.prv2_blend_resize_frames(p, p, 70000, 8, 8, p, p, 16, 16, None) != 0
    # frame strides that make frames overlap (mismatched counts): tile stride < k, prediction stride < k * ph * pw
    assert lib.prv2_blend_update_frames(p, p, 2, 32, 32, p, 8, 8, 4 * 64, p, p, 3, 4, 8, 8, None) != 0 and "stride" in _err(lib)
    assert lib.prv2_blend_paste_frames(p, p, 2, 32, 32, p, 8, 8, 4 * 64 - 1, p, p, 4, 4, 8, 8, None) != 0 and "stride" in _err(lib)
    # geometry: k < 1, knot spacing out of (0, 1/2], misaligned x2 output
    assert lib.prv2_roi_align_frames(p, 2, 8, 8, 4, 4, p, 0, 1.0, 4, 4, p, 4, None) != 0
    assert lib.prv2_coarse_tap_knots_frames(p, 2, 8, 8, 4, 36, 0.75, 0.25, p, 4, None) != 0 and "knot" in _err(lib)
    assert lib.prv2_roi_align_x2_frames(p, 2, 8, 8, 6, 8, p, 3, 1.0, 4, 4, p, 8, None) != 0
    assert lib.prv2_crop_resize_frames(p, 2, 64, 64, p, 3, 80, 32, 16, 16, m3, m3, p, 4, None) != 0 and "geometry" in _err(lib)
    with pytest.raises(RuntimeError):
        L.check(lib.prv2_blend_resize_frames(p, p, 0, 8, 8, p, p, 16, 16, None), "blend_resize_frames")


def test_frame_torch_ops_registered_and_reject_cpu_tensors():
    import torch
    from patchrefinerv2_amd import torch_ops
    ops = torch_ops.load()
    for name in FRAME_OPS:
        assert name in torch_ops.OPS
        getattr(ops, name).default._schema  # registered with a schema
    s = str(ops.roi_align_frames.default._schema)
    for frag in ("Tensor feat", "Tensor boxes", "float spatial_scale", "Tensor(a!)? out", "bool x2"):
        assert frag in s, (frag, s)
    assert "Tensor(a!) avg" in str(ops.blend_update_frames.default._schema)
    z = torch.zeros
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.crop_resize_frames(z(2, 3, 16, 16), z(3, 3, dtype=torch.int32), 8, 8, 8, 8)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.roi_align_frames(z(2, 4, 4, 4), z(3, 5), 1.0, 4, 4)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.coarse_tap_knots_frames(z(2, 4, 4, 36), 4, 0.25, 0.25)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.coarse_tap_gather_frames(z(2, 12, 12, 4), z(2, 4, 4, 36), 0.25, 0.25, z(3, 5), 1.0, 4, 4)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.blend_init_frames(z(2, 8, 8), z(2, 8, 8), z(2, 1, 4, 4), z(4, 4), z(2, 1, 2, dtype=torch.int32), 4, 4)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.blend_update_frames(z(2, 8, 8), z(2, 8, 8), z(2, 1, 4, 4), z(4, 4), z(2, 1, 2, dtype=torch.int32), 4, 4)
    with pytest.raises((NotImplementedError, RuntimeError)):
        ops.blend_resize_frames(z(2, 8, 8), z(2, 8, 8), 16, 16)


def _planner(kind, pps):
    from patchrefinerv2_amd import models as M
    cls = {"plus": M.PatchRefinerPlus, "baseline": M.BaselinePretrain}[kind]
    pl = object.__new__(cls)  # host-only: the planner needs the patch size, no weights and no device
    pl.patch_process_shape = tuple(pps)
    return pl


@pytest.mark.parametrize("kind", ["plus", "baseline"])
@pytest.mark.parametrize("mode", ["m1", "m2", "r8", "r32"])
def test_plan_frames_consumes_random_like_sequential_plans(kind, mode):
    pl = _planner(kind, (384, 512))
    tc = pl.prepare_tile_cfg([2160, 3840], [4, 4])
    for B in (1, 3, 4):
        random.seed(17)
        ref = [pl.plan_tiles(tc, mode, 4) for _ in range(B)]
        after_ref = random.random()
        random.seed(17)
        got = pl.plan_frames(tc, mode, 4, B)
        assert got == ref and random.random() == after_ref
        # frame_seeds: random.seed(frame_seeds[f]) right before frame f's plan, as a loop seeding every frame does
        seeds = [621 + 7 * f for f in range(B)]
        ref = []
        for s in seeds:
            random.seed(s)
            ref.append(pl.plan_tiles(tc, mode, 4))
        after_ref = random.random()
        random.seed(3)
        got = pl.plan_frames(tc, mode, 4, B, frame_seeds=seeds)
        assert got == ref and random.random() == after_ref
        # all frames share pass kinds and counts (one tile_cfg): only the r-mode positions differ
        assert len({tuple((p["kind"], len(p["raw"])) for p in plan) for plan in got}) == 1
    if mode[0] == "r":
        random.seed(17)
        two = pl.plan_frames(tc, mode, 4, 2)
        assert two[0][-1]["raw"] != two[1][-1]["raw"]  # the random tiles differ from frame to frame
    with pytest.raises(ValueError):
        pl.plan_frames(tc, mode, 4, 3, frame_seeds=[1, 2])
