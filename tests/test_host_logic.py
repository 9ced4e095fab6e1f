"""CPU: host-side logic of the product (tile planner, boxes, mask, config/registry) against the
golden vectors captured from the reference -- no GPU, no oracle in the product path."""
import json
import os
import random

import numpy as np
import pytest

from patchrefinerv2_amd import models as M
from patchrefinerv2_amd.registry import MODELS, Config, ConfigDict, build_model

GOLD = os.path.join(os.path.dirname(__file__), "golden")


class _Planner(M._PatchModel):
    def __init__(self, pps):
        super().__init__()
        self.patch_process_shape = tuple(pps)

    def _pack(self):
        pass


def test_tile_plans_match_reference():
    g = np.load(os.path.join(GOLD, "tiling.npz"))
    plans = json.load(open(os.path.join(GOLD, "tile_plans.json")))
    for name, p in plans.items():
        pl = _Planner(p["pps"])
        tc = pl.prepare_tile_cfg(p["raw"], p["split"])
        random.seed(621)
        passes = pl.plan_tiles(tc, p["mode"], 4)
        flat = [t for ps in passes for t in ps["raw"]]
        assert len(flat) == p["n"]
        rh, rw = tc["patch_raw_shape"]
        bb = np.array([[w, h, w + rw, h + rh] for h, w in flat], dtype=np.int32)
        assert np.array_equal(bb, g[f"plan_{name}_bboxs"])
        assert np.array_equal(pl._boxes(flat, tc), g[f"plan_{name}_bboxs_feat"][:, 1:])


def test_patch_counts():
    pl = _Planner((384, 512))
    tc = pl.prepare_tile_cfg([2160, 3840], [4, 4])
    for mode, n in (("m1", 16), ("m2", 49), ("r32", 81), ("r64", 113), ("r128", 177)):
        assert sum(len(p["raw"]) for p in pl.plan_tiles(tc, mode, 4)) == n
    assert tc["patch_reensemble_shape"] == (1536, 2048) and tc["patch_raw_shape"] == (540, 960)


def test_blend_mask_matches_reference_statistics():
    g = np.load(os.path.join(GOLD, "tiling.npz"))
    for (h, w) in ((384, 512), (448, 448), (540, 960)):
        mk = M.generatemask((h, w), border=0.15)
        np.testing.assert_allclose(mk.sum(axis=1), g[f"mask_{h}x{w}_rowsum"], rtol=2e-6, atol=1e-5)
        assert int((mk == 0).sum()) == int(g[f"mask_{h}x{w}_zeros"][0])


def test_registry_and_config(tmp_path):
    for t in ("PatchRefiner", "PatchRefinerPlus", "FusionUnet", "BiDirectionalFusion", "LightWeightRefiner", "SILogLoss"):
        assert t in MODELS
    with pytest.raises(KeyError):
        build_model(dict(type="NoSuchModel"))
    (tmp_path / "base.py").write_text("min_depth=1e-3\nmodel=dict(type='FusionUnet', input_chl=[8, 8], temp_chl=[4, 4], dec_chl=[4])\n")
    (tmp_path / "cfg.py").write_text("_base_=['base.py']\nmodel=dict(dec_chl=[8])\nextra=3\n")
    cfg = Config.fromfile(str(tmp_path / "cfg.py"))
    assert cfg.model.type == "FusionUnet" and cfg.model.dec_chl == [8] and cfg.min_depth == 1e-3 and cfg.extra == 3
    cfg.merge_from_dict({"model.temp_chl": [2, 2]})
    assert cfg.model.temp_chl == [2, 2]
    m = build_model(cfg.model)
    assert list(m.spec())[0] == "encoder_layers_1.0.single_conv.0.weight"
    assert isinstance(ConfigDict(a=dict(b=1)).a, ConfigDict)


def test_state_dict_contract_and_loud_failures():
    from oracle.cases import E2E_V2, e2e_v2_sd
    cfg = dict(E2E_V2["ref_config"])
    cfg["coarse_branch"] = dict(type="DA2", pretrained=None, model_cfg=dict(E2E_V2["da2_cfg"]))
    m = build_model(dict(type="PatchRefinerPlus", config=cfg))
    spec = m.spec()
    assert set(spec) == set(e2e_v2_sd().keys())
    assert "refiner_fine_branch.refiner_encoder.conv_stem.weight" in spec and spec[
        "refiner_fine_branch.refiner_encoder.conv_stem.weight"] == (32, 4, 3, 3)
    with pytest.raises(RuntimeError):
        m.load_state_dict({"bogus": 0}, strict=True)
    with pytest.raises(NotImplementedError):
        m(mode="train")
    bad = dict(cfg)
    bad["coarse_branch"] = dict(type="ZoeDepth")  # MidasCore / BEiT-L + ResizeZoe: only P = 384 x 512 can work (midas.py:171-174)
    with pytest.raises(ValueError):
        build_model(dict(type="PatchRefinerPlus", config=bad))
    bad["coarse_branch"] = dict(type="ZoeDepth", midas_model_type="DPT_SwinV2_L_384")
    with pytest.raises(NotImplementedError):
        build_model(dict(type="PatchRefinerPlus", config={**bad, "patch_process_shape": [384, 512]}))


def test_png16_and_read_image(tmp_path):
    from patchrefinerv2_amd.tester import ImageDataset, read_image, write_png16
    a = (np.arange(6 * 5).reshape(6, 5) * 1000).astype(np.uint16)
    write_png16(str(tmp_path / "x.png"), a)
    try:
        from PIL import Image
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / "x.png"))), a)
    except ImportError:
        pass
    img = np.random.RandomState(0).rand(20, 30, 3).astype(np.float32)
    np.save(str(tmp_path / "f.npy"), img)
    out = read_image(str(tmp_path / "f.npy"), "", (40, 60))
    import torch
    import torch.nn.functional as F
    ref = F.interpolate(torch.from_numpy(img).permute(2, 0, 1)[None], (40, 60), mode="bicubic", align_corners=True)
    assert np.allclose(out, ref[0].permute(1, 2, 0).numpy())
    os.remove(str(tmp_path / "x.png"))
    ds = ImageDataset(str(tmp_path), image_resolution=(40, 60))
    assert len(ds) == 1 and ds.files == ["f.npy"]  # (items are resized on the device: tests/test_hip_ops.py, test_cli.py)


def test_shipped_config_builds():
    cfg = Config.fromfile(os.path.join(os.path.dirname(os.path.dirname(__file__)), "configs", "v2_dav2_mobile_u4k.py"))
    m = build_model(cfg.model)
    assert m.tile_cfg["patch_raw_shape"] == (540, 960) and len(m.spec()) > 500


def test_m16_lds_layout_is_bank_conflict_free():
    """csrc/conv3x3_m16.hip: the 160-byte halo rows and the XOR-swizzled 128-byte weight rows give every
    ds_read_b128 lane group 16 distinct 16-byte bank slots, for every tap shift (MI355X_MICROARCH.md, LDS:
    ds_read_b128 is served in four 16-lane groups; a 16-byte slot = 4 of the 64 banks)."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
              [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[l + 32 for l in g] for g in groups]
    for plane in (0, 64):                                   # hi / lo plane of the halo row
        for p0 in range(34 * 3):                            # any halo pixel a 16-pixel run may start at
            for grp in groups:
                slots = {((p0 + (l & 15)) * 160 + plane + (l >> 4) * 16) // 16 % 16 for l in grp}
                assert len(slots) == 16
    for plane in (0, 4):                                    # weight rows: slot (g + plane) ^ ((row >> 1) & 7)
        for n0 in range(0, 128, 16):
            for grp in groups:
                slots = set()
                for l in grp:
                    row, g = n0 + (l & 15), l >> 4
                    slots.add((row * 128 + (((g + plane) ^ ((row >> 1) & 7)) << 4)) // 16 % 16)
                assert len(slots) == 16


def test_output_stage_matches_reference():
    """colour maps + evaluation metrics (patchrefinerv2_amd/metrics.py) vs the reference's own functions
    (estimator/utils/color.py, metric.py -> tests/golden/output_stage.npz by oracle/make_golden.py)."""
    import torch
    from patchrefinerv2_amd import metrics as M
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "output_stage.npz"))
    gt, pred, pred_lo, edges = (torch.from_numpy(g[k]) for k in ("gt", "pred", "pred_lo", "edges"))
    np.testing.assert_array_equal(M.colorize(pred.clone(), cmap="Spectral", vminp=0, vmaxp=100), g["color_spectral"])
    vv = gt.clone()
    vv[0, 0, :4, :4] = -99
    np.testing.assert_array_equal(M.colorize(vv, cmap="gray_r"), g["color_gray"])
    np.testing.assert_array_equal(M.get_boundaries(1.0 / gt.squeeze().numpy() * 40, th=1, dilation=0), g["edges"])
    e = M.compute_errors(gt.squeeze().numpy()[2:30, 2:40], np.abs(pred.squeeze().numpy()[2:30, 2:40]) + 0.01)
    for k, v in e.items():   # (the slice contains the NaN / inf pixels on purpose: NaN must propagate identically)
        np.testing.assert_equal(float(v), float(g[f"err_{k}"]), k)
    m1 = M.compute_metrics(gt, pred.clone(), garg_crop=False, eigen_crop=False, dataset="u4k", min_depth_eval=0.1,
                           max_depth_eval=10, disp_gt_edges=edges)
    m2 = M.compute_metrics(gt, pred_lo.clone(), garg_crop=True, eigen_crop=False, dataset="kitti", min_depth_eval=0.1,
                           max_depth_eval=10)
    for tag, m in (("m1", m1), ("m2", m2)):
        for k, v in m.items():
            np.testing.assert_equal(float(v), float(g[f"{tag}_{k}"]), f"{tag} {k}")
    # the device-side restatement (torch ops; runs on whatever device the tensors live on) agrees with the pinned host version
    d1 = M.compute_metrics_device(gt, pred.clone(), garg_crop=False, eigen_crop=False, dataset="u4k", min_depth_eval=0.1, max_depth_eval=10,
                                  disp_gt_edges=edges)
    d2 = M.compute_metrics_device(gt, pred_lo.clone(), garg_crop=True, eigen_crop=False, dataset="kitti", min_depth_eval=0.1, max_depth_eval=10)
    for ref, got in ((m1, d1), (m2, d2)):
        assert set(ref) == set(got)
        for k in ref:
            np.testing.assert_allclose(float(got[k]), float(ref[k]), rtol=2e-5, atol=1e-7, err_msg=k)
    np.testing.assert_array_equal(M.soft_edge_error(np.abs(pred.squeeze().numpy()), gt.squeeze().numpy(), radius=2), g["see_r2"])
    with pytest.raises(NotImplementedError):
        M.get_boundaries(gt.squeeze().numpy(), dilation=3)


REFERENCE_CONFIG_FLOOR = 80  # raised as components land; see the printed table (the 19 PatchRefinerSemi configs build their student: inference-only wrapper)


def test_reference_model_configs_build_through_the_registry():
    """SURVEY.md 8(b) 'Registry': the ``model=dict(type=..., ...)`` section of every config the reference ships
    (tests/golden/reference_model_configs.json, generated by oracle/make_config_fixture.py) goes through the product's
    MODELS.build.  Out of scope by SURVEY.md 2: PatchFusion (predecessor, 2), pretrain_stage=True (training).  PatchRefinerSemi (19
    configs) builds as its inference-only delegate to the student.  Prints what builds and why the rest does not."""
    import collections
    import json
    import os
    import warnings
    from patchrefinerv2_amd import models  # noqa: F401
    from patchrefinerv2_amd.registry import build_model
    with open(os.path.join(os.path.dirname(__file__), "golden", "reference_model_configs.json")) as f:
        cfgs = json.load(f)
    ok, fails = [], collections.defaultdict(list)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # "checkpoint ... does not exist -- skipped" (the configs name the authors' local paths)
        for rel, mc in cfgs.items():
            try:
                build_model(mc)
                ok.append(rel)
            except (NotImplementedError, KeyError) as e:
                fails[f"{type(e).__name__}: {str(e)[:100]}"].append(rel)
    print(f"\n{len(ok)} of {len(cfgs)} reference model configs build")
    for k, v in sorted(fails.items(), key=lambda kv: -len(kv[1])):
        print(f"  {len(v):3d}  {k}")
    assert len(cfgs) == 99
    assert len(ok) >= REFERENCE_CONFIG_FLOOR, (len(ok), dict(fails))


def test_canny_edge_map_of_the_output_stage():
    """<name>_edge.png (tester.py:99-106): Canny of the log depth + 3 x 3 dilation.  skimage / kornia are absent: the detector
    is a restatement on scipy.ndimage (parity unpinned); checked on shapes whose edges are known."""
    import torch
    from patchrefinerv2_amd.metrics import canny, depth_edges
    img = np.zeros((64, 96), np.float32)
    img[:, 40:] = 1.0
    yy, xx = np.mgrid[:64, :96]
    img[(yy - 32) ** 2 + (xx - 20) ** 2 < 100] = 2.0
    e = canny(img)
    assert e.dtype == bool and e[5:60, 39:41].all() and not e[:, 50:90].any() and not e[:, :5].any()
    ring = np.hypot(yy - 32, xx - 20)
    assert e[(ring > 8) & (ring < 12)].sum() > 40 and not e[ring < 7].any()
    assert not canny(np.full((32, 32), 3.0, np.float32)).any()            # constant image: the zero border is corrected for
    d = depth_edges(torch.tensor(np.exp(img))[None, None])
    assert d.shape == (64, 96) and d.sum() > e.sum() and (d | ~e).all()    # dilation contains the thin edges


def test_checkpoint_key_remap_and_diagnosis():
    """checkpoint readiness (patchrefinerplus.py:105-124,202-205): a state dict saved with a DDP prefix, timm's FLATTENED feature-net
    names and BatchNorm bookkeeping buffers is rewritten onto this build's table; what cannot be explained is reported grouped by
    module with rename candidates"""
    import re
    import torch
    from patchrefinerv2_amd import weights as W
    spec = W.mnv4_spec("refiner_fine_branch.refiner_encoder.", in_chans=4)
    spec["refiner_fusion_model.final_conv.weight"] = (1, 32, 3, 3)
    sd = {k: torch.zeros(shp) for k, shp in spec.items()}
    odd = {}
    for k, v in sd.items():
        k2 = "module." + re.sub(r"\.blocks\.(\d+)\.", r".blocks_\1.", k)
        odd[k2] = v
        if k.endswith("running_var"):
            odd[k2.replace("running_var", "num_batches_tracked")] = torch.zeros(())
    odd["module.refiner_fusion_model.final_conv.weight"] = odd.pop("module.refiner_fusion_model.final_conv.weight")
    new, applied = W.remap_state_dict(odd, spec)
    assert sorted(new) == sorted(spec) and applied["DistributedDataParallel prefix"] == len(spec)
    assert applied["dropped bookkeeping buffers"] > 0 and applied["timm FeatureListNet flattening (blocks_N -> blocks.N)"] > 100
    # an unknown naming: reported, with the right rename candidate
    bad = dict(sd)
    v = bad.pop("refiner_fine_branch.refiner_encoder.conv_stem.weight")
    bad["refiner_fine_branch.refiner_encoder.stem.conv.weight"] = v
    bad["totally.unrelated"] = torch.zeros(3)
    new, applied = W.remap_state_dict(bad, spec)
    d = W.diagnose_state_dict(spec, new)
    assert d["matched"] == len(spec) - 1 and list(d["missing"]) == ["refiner_fine_branch.refiner_encoder.conv_stem.weight"]
    assert d["rename_candidates"]["refiner_fine_branch.refiner_encoder.stem.conv.weight"] == ["refiner_fine_branch.refiner_encoder.conv_stem.weight"]
    txt = W.format_diagnosis(d)
    assert "MISSING" in txt and "UNEXPECTED" in txt and "totally" in txt and "rename candidates" in txt


def test_split_arithmetic_study_orders_the_schemes():
    """tools/studies/split_arith_study.py (numpy emulation against float64): bf16x3 -- the shipped arithmetic --
    is fp32-grade (< 1e-5 per dot product), and the candidate of the next round, one fp16 product + two block-scaled e2m3 corrections,
    stays within 4 x of it and 15 x under a single fp16 product"""
    import importlib.util
    import os
    import numpy as np
    spec = importlib.util.spec_from_file_location("split_arith_study", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "studies",
                                                                                    "split_arith_study.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((32, 1152)).astype(np.float32)
    w = (rng.standard_normal((48, 1152)) / 34.0).astype(np.float32)
    ref, out = mod.dots(x, w)
    den = np.sqrt((ref ** 2).mean())
    err = {k: float(np.sqrt(((v - ref) ** 2).mean()) / den) for k, v in out.items()}
    assert err["bf16x3"] < 1e-5 < err["f16"] and err["bf16"] > 1e-3
    assert err["f16+f6x2"] < 4 * err["bf16x3"] and err["f16+f6x2"] * 15 < err["f16"]
    assert err["f16+f6x2"] <= err["f16+f8x2"] < err["f16+f4x2"]


def test_upconv_algebra_conv_of_upsample_equals_gathered_tap_gemms():
    """The identity csrc/upconv.hip computes (prv2_upconv3x3), in float64 on the CPU with the kernel's own index arithmetic:
        conv3x3(interpolate(u, (H, W), 'bilinear', align_corners=True); W)(p) = sum_tap [p + d_tap inside the image] Bil(G_tap; s(p + d_tap)),
        G_tap = W[:, :, tap] . u  (a 1x1 GEMM at u's resolution)
    -- the channel contraction commutes with the interpolation; the zero padding of the conv applies to the OUTPUT grid (a tap outside
    the image contributes nothing), not to the source.  bi_directional_fusion_model.py:139-142,201; fusion_model.py:15-24.  Also the two
    bounds the kernel's tile shape relies on for a source step <= 1/2 pixel: consecutive output pixels advance the source column by at
    most one, and a 16 x 28 output tile with its one-pixel tap ring touches at most 11 x 17 source pixels."""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(7)

    def ac_tap(dst, scale, n_in):  # common.h::ac_tap in float32, as the kernels evaluate it
        src = np.float32(scale) * np.float32(dst)
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        w1 = float(np.float32(src) - np.float32(i0))
        return i0, i1, 1.0 - w1, w1

    for (h, w, H, W, cin, cout) in [(5, 7, 10, 14, 3, 4), (6, 5, 11, 9, 2, 3), (4, 4, 16, 13, 2, 2)]:
        u = torch.randn(1, cin, h, w, generator=g, dtype=torch.float64)
        wt = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
        ref = F.conv2d(F.interpolate(u, (H, W), mode="bilinear", align_corners=True), wt, padding=1)[0]
        sy = np.float32((h - 1) / (H - 1)) if H > 1 else np.float32(0)
        sx = np.float32((w - 1) / (W - 1)) if W > 1 else np.float32(0)
        G = torch.einsum("oikl,ihw->klohw", wt, u[0])  # [ky, kx, cout, h, w]: the nine tap GEMMs
        got = torch.zeros(cout, H, W, dtype=torch.float64)
        for y in range(H):
            for x in range(W):
                for ky in range(3):
                    for kx in range(3):
                        yy, xx = y + ky - 1, x + kx - 1
                        if not (0 <= yy < H and 0 <= xx < W):
                            continue  # the conv's zero padding: this tap sees nothing
                        r0, r1, wy0, wy1 = ac_tap(yy, sy, h)
                        c0, c1, wx0, wx1 = ac_tap(xx, sx, w)
                        t = G[ky, kx]
                        got[:, y, x] += wy0 * (wx0 * t[:, r0, c0] + wx1 * t[:, r0, c1]) + wy1 * (wx0 * t[:, r1, c0] + wx1 * t[:, r1, c1])
        # float32 source coordinates against torch's float64 ones: ~1e-7 relative, the same difference the HIP upsample kernel has
        assert float((got - ref).abs().max()) < 5e-6 * max(1.0, float(ref.abs().max())), (h, w, H, W)
    # footprint bounds of a 16 x 28 tile (csrc/upconv.hip: LR = 11, LC = 17) for every tile origin of a x2 upsample and of the 2n - 1 corner case
    # ... and of a 14 x 24 tile for a source step up to 3/5 (DepthAnything's 256 -> 448)
    for (n_in, n_out) in [(192, 384), (256, 512), (9, 17), (24, 48), (100, 199), (256, 448), (16, 28), (4, 6)]:
        s = np.float32((n_in - 1) / (n_out - 1))
        i0 = [ac_tap(min(max(d, 0), n_out - 1), s, n_in)[0] for d in range(-1, n_out + 1)]
        assert all(0 <= b - a <= 1 for a, b in zip(i0, i0[1:]))
        for span, bound in (((16, 11), (28, 17)) if s <= 0.5 else ((14, 11), (24, 17))):
            for o in range(0, n_out, span):
                lo, hi = i0[o], i0[min(o + span + 1, len(i0) - 1)]   # taps o - 1 .. o + span
                assert hi - lo + 2 <= bound, (n_in, n_out, span, o, lo, hi)


def test_composite_5x5_of_the_two_linear_convs_behind_the_upsample():
    """Groundwork for DESIGN.md section 9 item 0a (tools/studies/composite5x5_study.py): output_conv2[0] o output_conv1 o interpolate
    (bi_directional_fusion_model.py:139-146,201-203) == ONE 5x5 conv of the upsampled map + a nine-valued bias map - a fix on the one-pixel
    border ring, exactly (float64), for the real channel ratio too (fewer MACs: 25 cin c2 against 9 cin c1 + 9 c1 c2)"""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("c5", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "studies", "composite5x5_study.py"))
    c5 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(c5)
    g = torch.Generator().manual_seed(3)
    for (cin, c1, c2, h, w) in [(8, 6, 4, 9, 11), (16, 8, 2, 5, 6)]:
        u = torch.randn(1, cin, h, w, generator=g, dtype=torch.float64)
        w1, b1 = torch.randn(c1, cin, 3, 3, generator=g, dtype=torch.float64) / 8, torch.randn(c1, generator=g, dtype=torch.float64)
        w2, b2 = torch.randn(c2, c1, 3, 3, generator=g, dtype=torch.float64) / 7, torch.randn(c2, generator=g, dtype=torch.float64)
        r = c5.composite(u, w1, b1, w2, b2, (2 * h, 2 * w))
        assert r["err"] < 1e-12 * max(1.0, r["scale"]), r
        assert r["ring_pixels"] == 2 * (2 * h + 2 * w) - 4 and r["bias_vectors"] == 9 and r["err_without_ring_fix"] > 1e-3, r
    assert 25 * 256 * 32 < 9 * 256 * 128 + 9 * 128 * 32   # the real layer pair: 204.8 k against 331.8 k MACs per output pixel


def test_bidir_fusion_c2f_types_spec_and_refusal():
    """The parameter tables of the three C2FModule types built here (bi_directional_fusion_model.py:355-372) and the loud refusal of
    the fourth ('only-gate', C2FNOENCModule)"""
    from patchrefinerv2_amd import weights as W
    from patchrefinerv2_amd.fusion import BiDirectionalFusion
    a = (list((32, 256, 256, 256, 256, 256)), [32, 32, 64, 96, 960], [32, 256, 256, 256, 256, 256], [32, 64, 64, 128, 256, 512],
         [512, 256, 128, 64, 32])
    gated = W.bidir_fusion_spec("", *a)
    assert gated == W.bidir_fusion_spec("", *a, coarse2fine_type="coarse-fusion")
    plain = W.bidir_fusion_spec("", *a, coarse2fine_type="self-agg")
    assert {k for k in gated if k not in plain} == {k for k in gated if ".fusion_conv." in k} and len(plain) == len(gated) - 12 * 5
    og = W.bidir_fusion_spec("", *a, coarse2fine_type="only-gate")  # C2FNOENCModule: 12 units, ConvTranspose stem, no refinenet blocks
    assert sum(k.endswith("_gate1.conv.weight") or k.endswith("_gate2.conv.weight") for k in og) == 12 and not any("refinenet" in k for k in og)
    assert og["c2f.scratch.upsample_conv.0.weight"] == (32, 32, 2, 2) and og["c2f.scratch.output_conv.weight"] == (1, 32, 3, 3)
    with pytest.raises(NotImplementedError, match="coarse2fine_type"):
        BiDirectionalFusion(coarse2fine_type="no-such-type", device="cpu")
    with pytest.raises(NotImplementedError, match="glb_att"):
        BiDirectionalFusion(glb_att=True, device="cpu")


def test_lds_layouts_by_the_bank_model():
    """tools/lds_bank_model.py (the per-instruction lane groups / bank moduli of MI355X_MICROARCH.md, LDS): the layouts fixed in round 4 are
    conflict free in the model, and the model reproduces what SQ_LDS_BANK_CONFLICT showed for their predecessors (r04_experiments.txt #19-21)"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("lds_bank_model", os.path.join(os.path.dirname(__file__), "..", "tools", "lds_bank_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    r = m.report()
    assert r["a_fragment_read_arow160"] == 0 and r["a_fragment_read_arow144"] > 0
    assert r["upconv_walk_read"] == 0 and r["upconv_walk_read_old_roles"] > 0
    assert r["gate_gemm_read"] == 0 and r["gate_gemm_read_identity_rows"] > 0
    assert r["halo16_epilogue_read_bn128"] == 0 and r["halo16_epilogue_read_bn32"] > 0 and r["halo16_epilogue_read_bn64"] > 0  # natural roles
    assert r["halo16_store_loop_read_bn32"] == 0 and r["halo16_store_loop_read_bn64"] == 0                                     # shipped roles
    for bn in (32, 64, 128):
        assert sorted(m.halo16_store_role(bn, t) for t in range(512)) == [(r_, q) for r_ in range(512 // (bn // 4)) for q in range(bn // 4)] or bn == 128
        assert r[f"ln_stats_read_b128_bn{bn}"] == 0 and r[f"ln_stats_read_b32_bn{bn}"] >= 6  # 16-byte reads: free; scalar: 4-way per half
    assert sorted(m.upconv_gather_role(l) for l in range(64)) == [(r_, q) for r_ in range(8) for q in range(8)]
    assert sorted(m.gate_gemm_row(i) for i in range(16)) == list(range(16))
    # round 5, csrc/conv3x3_f6.hip: the halo image's pitch and the split of an fp6 block into two 16-byte column groups
    assert r["f6_fragment_read_pix288"] == 0 and r["f6_fragment_read_pix272"] > 0 and r["f6_fragment_read_blocks_contiguous"] > 0
    assert r["f6_epilogue_row_write"] == 0
    f6 = open(os.path.join(os.path.dirname(__file__), "..", "patchrefinerv2_amd", "csrc", "conv3x3_f6.hip")).read()
    assert "constexpr int PIX = 288;" in f6 and "constexpr int RP = 1040;" in f6 and "ST_CHUNK = 1040" in f6
    # the constants of the kernels are the ones the model was run with
    src = open(os.path.join(os.path.dirname(__file__), "..", "patchrefinerv2_amd", "csrc", "upconv.hip")).read()
    assert "constexpr int AROW = 160;" in src and "0xD728" in src and "constexpr int GRP = LC * CLD - 4;" in src


def test_f6_range_guard_logic_on_cpu():
    """ops.F6Range (the fp16 range guard of the f16f6 mode) without a GPU: the table on the CPU device, the words written by hand -- which
    maxima trigger a recomputation, where the power-of-two scale goes, slots of dead layers are reused"""
    import struct
    import torch
    from patchrefinerv2_amd import ops

    class Layer:  # (stands for ops.ConvWF6: the guard only touches x_scale / range)
        x_scale = 1.0
        range = None

    bits = lambda v: struct.unpack("<i", struct.pack("<f", v))[0]  # noqa: E731
    a, b, c = Layer(), Layer(), Layer()
    for l in (a, b, c):
        l.range = ops.F6Range.slot("cpu", l)
    assert ops.F6Range.active("cpu")
    a.range[0], b.range[0], c.range[0] = bits(3.5), bits(4.0e5), bits(3.0e-8)
    redo = ops.F6Range.check("cpu")
    assert [r[0] for r in redo] == [b, c] and a.x_scale == 1.0                   # 3.5: fine; 4e5 > 65504 and 3e-8 < 2^-10: recompute
    assert b.x_scale == 2.0 ** (8 - 18) and c.x_scale == 2.0 ** (8 + 25)        # 2^18 <= 4e5 < 2^19 -> 2^8; 2^-25 <= 3e-8 < 2^-24 -> 2^8
    assert int(a.range[0]) == 0 and not ops.F6Range.check("cpu")                 # cleared for the next frame
    a.range[0] = bits(20000.0)                                                  # inside fp16, but within two binades of its end: moved, not recomputed
    assert ops.F6Range.check("cpu") == [] and a.x_scale == 2.0 ** (8 - 14)
    slot_b = b.range.data_ptr()
    del b, redo
    import gc
    gc.collect()
    d = Layer()
    d.range = ops.F6Range.slot("cpu", d)
    assert d.range.data_ptr() == slot_b                                          # a dead layer's slot is handed out again


def test_winograd_f23_study_identity_and_error_growth():
    """tools/studies/winograd_f23_study.py (the next algebraic lever): the F(2x2, 3x3) identity holds in float64 and the transforms cost the
    split-operand arithmetics less than 2x in rms error -- bf16x3 Winograd stays below the fp16 + fp6 direct conv's error"""
    import importlib.util
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("winograd_f23_study", os.path.join(root, "tools", "studies", "winograd_f23_study.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    rng = np.random.default_rng(1)
    x = np.maximum(rng.standard_normal((10, 18, 64)), 0).astype(np.float32)
    w = (rng.standard_normal((16, 64, 3, 3)) / 24).astype(np.float32)
    ref = m.direct(x, w, "exact")
    den = np.sqrt((ref ** 2).mean())
    assert np.abs(m.winograd(x, w, "exact") - ref).max() < 1e-5 * den
    err = {(k, mode): np.sqrt(((f(x, w, mode) - ref) ** 2).mean()) / den for k, f in (("direct", m.direct), ("winograd", m.winograd)) for mode in ("bf16x3", "f16f6")}
    assert err[("winograd", "bf16x3")] < 2.0 * err[("direct", "bf16x3")] < 1.2e-5
    assert err[("winograd", "f16f6")] < 2.0 * err[("direct", "f16f6")] and err[("winograd", "bf16x3")] < err[("direct", "f16f6")]


def test_conv_desc_and_ups_src_fill_every_field_of_the_c_structs():
    """ops._conv_desc / ops._ups_src are the only places that build prv2_conv_desc / prv2_ups_src: every field of the two ctypes structs
    (iterated from ``_fields_``: a field added later fails here until it is listed) for the keyword sets of the five kinds of caller"""
    from types import SimpleNamespace

    from patchrefinerv2_amd import lib as L
    from patchrefinerv2_amd import ops
    x = SimpleNamespace(n=2, h=20, w=33, c=34, ld=36, ptr=0x7000)
    cw = ops.ConvW(w=None, bias=None, cout=40, cin=34, kh=3, kw=5, stride=2, pad=1, convt_k=0, prec=L.PREC_BF16X3, same_pad=True)
    base = dict(n=2, h=20, w=33, cin=34, cout=40, kh=3, kw=5, stride=2, pad=1, ldx=36, ldy=44, x_bstride=0, y_bstride=0, relu_in=0, act=0, convt_k=0,
                ld_mul=0, ld_res=0, ld_res2=0, prec=1, force_generic=0, ln_eps=float(np.float32(1e-6)), part=0, same_pad=1, fmt=0)
    eps = 2.0 ** -10
    callers = {
        "supported": (dict(), base),
        "conv2d": (dict(act=ops.ACT_GELU, relu_in=True, ld_mul=48, ld_res=52, ld_res2=56, ln_eps=eps, x_bstride=1 << 33, force_generic=True),
                   dict(base, act=2, relu_in=1, ld_mul=48, ld_res=52, ld_res2=56, ln_eps=eps, x_bstride=1 << 33, force_generic=1)),
        "conv2d_ups": (dict(act=ops.ACT_RELU, ld_res=52, ln_eps=eps), dict(base, act=1, ld_res=52, ln_eps=eps)),
        "conv2d_tail": (dict(act=ops.ACT_SILU, ln_eps=eps), dict(base, act=5, ln_eps=eps)),
        "conv2d_pre": (dict(act=ops.ACT_SIGMOID, ld_res=44, ln_eps=eps), dict(base, act=3, ld_res=44, ln_eps=eps)),
        "conv3x3_ln_gate": (dict(act=ops.ACT_RELU, relu_in=True, ld_mul=256, ld_res=260, ln_eps=eps, fmt=L.FMT_X_X2 | L.FMT_MUL_X2),
                            dict(base, act=1, relu_in=1, ld_mul=256, ld_res=260, ln_eps=eps, fmt=3)),
    }
    names = [name for name, _ in L.ConvDesc._fields_]
    assert sorted(names) == sorted(base)
    for caller, (kw, want) in callers.items():
        d = ops._conv_desc(x, cw, 44, **kw)
        for name in names:
            assert getattr(d, name) == want[name], (caller, name)
    # the fp16 + fp6 layers: a ConvWF6 has one layer shape
    d = ops._conv_desc(x, ops.ConvWF6(None, None, 256, 64, 1.0), 256, relu_in=True, ld_res=260, fmt=L.FMT_Y_X2)
    want = dict(base, cin=64, cout=256, kh=3, kw=3, stride=1, pad=1, ldy=256, relu_in=1, ld_res=260, prec=3, same_pad=0, fmt=4)
    for name in names:
        assert getattr(d, name) == want[name], ("conv3x3_f6", name)
    assert ops._gate_fmt(SimpleNamespace(x2=True), SimpleNamespace(x2=True)) == 3 and ops._gate_fmt(SimpleNamespace(x2=True)) == 1
    assert ops._gate_fmt(x, SimpleNamespace(x2=False)) == 0

    u = SimpleNamespace(n=2, h=10, w=17, c=32, ld=36, ptr=0x7000)
    us, want = ops._ups_src(u), dict(x=0x7000, h=10, w=17, ld=36, channels=32, bstride=0)
    names = [name for name, _ in L.UpsSrc._fields_]
    assert sorted(names) == sorted(want)
    for name in names:
        assert getattr(us, name) == want[name], name
