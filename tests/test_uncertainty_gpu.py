"""GPU: overlap statistics (``return_uncertainty``).  The prv2_blend_*_stats ops against a float64 restatement of their definition (both
dispatch routes, B = 1 and B = 3), with avg / cnt bit-equal to the blend without statistics; the models' ``uncertainty`` / ``count_map``
against the same restatement driven by ``predict_tiles`` on the plan's tiles, depth bit-equal to a call without the flag; B frames,
captured hipGraphs and f16f6; the rejected modes; ``tools/test.py --generate-pl`` end to end.

Tolerance of the uncertainty u against the float64 restatement u64: max|u - u64| <= 1e-4 * max(u64) + 1e-6 * max|a|.  The kernel keeps
m2 in fp32 with at most a few dozen sequential updates per pixel: m2's own rounding is a relative error of a few dozen ulp (2^-24 each),
i.e. far below 1e-4 of u; the running mean it is taken around is rounded to fp32 at every update, so each deviation p - a carries an
absolute error of about (updates) x 2^-24 x |a| <= 1e-6 |a|, which moves the weighted standard deviation by at most as much.
"""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.cases import E2E_V1, E2E_V2, e2e_v1_sd, e2e_v2_sd, rand_image  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
torch.set_grad_enabled(False)
F32 = np.float32


@pytest.fixture(params=["ctypes", "torch"])
def route(request, monkeypatch):
    from patchrefinerv2_amd import ops
    ops.L.load()
    monkeypatch.setattr(ops, "DISPATCH", request.param)
    return ops


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------------------------
# float64 restatement of the overlap statistics (the sampling indices and resize taps in the kernels' fp32 index arithmetic)
# ------------------------------------------------------------------------------------------------------------------------------
def _nearest(n_out, n_in):
    """legacy 'nearest' source index: min(floor(dst * float32(in / out)), in - 1)"""
    scale = F32(n_in) / F32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=F32) * scale).astype(np.int64), n_in - 1)


def _ac_taps(n_out, n_in):
    """bilinear align_corners=True taps (i0, i1, w0, w1) in fp32 index arithmetic"""
    scale = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
    src = np.arange(n_out, dtype=F32) * scale
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    w1 = (src - i0.astype(F32)).astype(np.float64)
    return i0, i1, 1.0 - w1, w1


class Ref64:
    """avg / cnt / m2 / ntiles of one frame in float64, exactly as the definition reads"""

    def __init__(self, h, w):
        self.a, self.c, self.s, self.n = (np.zeros((h, w)) for _ in range(4))

    @staticmethod
    def _sample(pred, th, tw):
        ph, pw = pred.shape
        iy = np.arange(th) if ph == th else _nearest(th, ph)
        ix = np.arange(tw) if pw == tw else _nearest(tw, pw)
        return pred[np.ix_(iy, ix)].astype(np.float64)

    def paste(self, preds, mask, tiles, th, tw):
        for pred, (h, w) in zip(preds, tiles):
            sl = (slice(h, h + th), slice(w, w + tw))
            self.a[sl], self.c[sl], self.s[sl], self.n[sl] = self._sample(pred, th, tw), mask, 0.0, 1.0

    def update(self, preds, mask, tiles, th, tw):
        ct = mask.astype(np.float64)
        for pred, (h, w) in zip(preds, tiles):
            sl = (slice(h, h + th), slice(w, w + tw))
            p, a, c, s = self._sample(pred, th, tw), self.a[sl], self.c[sl], self.s[sl]
            self.n[sl] += 1.0
            d = p - a
            a_new = (p * ct + c * a) / np.where(ct > 0, c + ct, 1.0)
            on = ct > 0
            self.s[sl] = np.where(on, s + ct * d * (p - a_new), s)
            self.a[sl] = np.where(on, a_new, a)
            self.c[sl] = np.where(on, c + ct, c)

    def resize(self, oh, ow):
        H, W = self.a.shape
        iy, ix = _nearest(oh, H), _nearest(ow, W)
        y0, y1, wy0, wy1 = _ac_taps(oh, H)
        x0, x1, wx0, wx1 = _ac_taps(ow, W)
        c = self.c
        c_o = wy0[:, None] * (wx0[None] * c[np.ix_(y0, x0)] + wx1[None] * c[np.ix_(y0, x1)]) + \
            wy1[:, None] * (wx0[None] * c[np.ix_(y1, x0)] + wx1[None] * c[np.ix_(y1, x1)])
        c_s, s_s = c[np.ix_(iy, ix)], self.s[np.ix_(iy, ix)]
        v = np.where(c_s > 0, s_s / np.where(c_s > 0, c_s, 1.0), 0.0)
        self.a, self.n, self.c, self.s = self.a[np.ix_(iy, ix)], self.n[np.ix_(iy, ix)], c_o, v * c_o

    def uncertainty(self):
        return np.where(self.c > 0, np.sqrt(np.maximum(self.s, 0.0) / np.where(self.c > 0, self.c, 1.0)), 0.0)


def _check_u(u, ref, a_scale):
    u = np.asarray(u, dtype=np.float64)
    u64 = ref.uncertainty()
    err = float(np.abs(u - u64).max())
    bound = 1e-4 * float(u64.max()) + 1e-6 * a_scale
    assert err <= bound, (err, bound)
    return u64


# ------------------------------------------------------------------------------------------------------------------------------
# ops
# ------------------------------------------------------------------------------------------------------------------------------
H0, W0, PH, PW, OH, OW, RH, RW = 24, 32, 12, 16, 36, 48, 18, 24
GRID = [(0, 0), (0, 16), (12, 0), (12, 16)]
HALF = [(0, 8), (6, 0), (6, 8), (6, 16), (12, 8)]


def _op_inputs(B, seed):
    mask = torch.rand(PH, PW, generator=_g(seed)).to(DEV)
    mask[:2] = 0          # zero bands: pasted pixels of weight 0, updates that only count
    mask[:, -3:] = 0
    mask_r = (torch.rand(RH, RW, generator=_g(seed + 1)) + 1e-3).to(DEV)
    mask_r[-2:] = 0
    n1, n2, n3 = len(GRID), len(HALF), 6
    n = n1 + n2 + n3
    preds = (torch.rand(B, n, PH, PW, generator=_g(seed + 2)) * 10 + 1).to(DEV)
    gen = np.random.RandomState(seed + 3)
    rnd = [[(int(gen.randint(0, OH - RH + 1)), int(gen.randint(0, OW - RW + 1))) for _ in range(n3)] for _ in range(B)]
    proc = torch.tensor([GRID + HALF + rnd[f] for f in range(B)], dtype=torch.int32).to(DEV)  # [B, n, 2] frame-major
    return mask, mask_r, preds, proc, (n1, n2, n3), rnd


def _ref_frame(f, mask, mask_r, preds, rnd, counts):
    n1, n2, n3 = counts
    pr = preds[f].cpu().numpy()
    m, mr = mask.cpu().numpy().astype(np.float64), mask_r.cpu().numpy().astype(np.float64)
    ref = Ref64(H0, W0)
    ref.paste(pr[:n1], m, GRID, PH, PW)
    ref.update(pr[n1:n1 + n2], m, HALF, PH, PW)
    ref.resize(OH, OW)
    ref.update(pr[n1 + n2:], mr, rnd[f], RH, RW)
    return ref


def test_blend_stats_single_frame_against_float64(route):
    """B = 1 ([H, W] maps): paste, half-offset grid updates, resize, random updates of another tile size (nearest-sampled predictions)"""
    ops = route
    mask, mask_r, preds, proc, (n1, n2, n3), rnd = _op_inputs(1, 20)
    pr, pt = preds[0], proc[0]
    maps = [torch.zeros(H0, W0, device=DEV) for _ in range(4)]
    avg, cnt = torch.zeros(H0, W0, device=DEV), torch.zeros(H0, W0, device=DEV)
    ops.blend_paste_stats(*maps, pr[:n1], mask, pt[:n1].contiguous(), PH, PW)
    ops.blend_paste(avg, cnt, pr[:n1], mask, pt[:n1].contiguous(), PH, PW)
    ops.blend_update_stats(*maps, pr[n1:n1 + n2], mask, pt[n1:n1 + n2].contiguous(), PH, PW)
    ops.blend_update(avg, cnt, pr[n1:n1 + n2], mask, pt[n1:n1 + n2].contiguous(), PH, PW)
    assert torch.equal(maps[0], avg) and torch.equal(maps[1], cnt)
    maps = list(ops.blend_resize_stats(*maps, OH, OW))
    avg, cnt = ops.blend_resize(avg, cnt, OH, OW)
    assert torch.equal(maps[0], avg) and torch.equal(maps[1], cnt)
    ops.blend_update_stats(*maps, pr[n1 + n2:], mask_r, pt[n1 + n2:].contiguous(), RH, RW)
    ops.blend_update(avg, cnt, pr[n1 + n2:], mask_r, pt[n1 + n2:].contiguous(), RH, RW)
    assert torch.equal(maps[0], avg) and torch.equal(maps[1], cnt)
    ref = _ref_frame(0, mask, mask_r, preds, rnd, (n1, n2, n3))
    assert np.array_equal(maps[3].cpu().numpy(), ref.n)
    u64 = _check_u(ops.blend_uncertainty(maps[1], maps[2]).cpu(), ref, float(avg.abs().max()))
    assert u64.max() > 0.1 and int(ref.n.max()) >= 3  # real overlap, real spread


def test_blend_stats_frames_against_float64_and_single_frame(route):
    """B = 3: each pass step one launch for all frames, frame f's tiles a strided slice of a frame-major list; every frame equals the B = 1
    statistics ops bit for bit and the restatement within the bound"""
    ops = route
    B = 3
    mask, mask_r, preds, proc, (n1, n2, n3), rnd = _op_inputs(B, 40)
    maps = [torch.zeros(B, H0, W0, device=DEV) for _ in range(4)]
    avg, cnt = torch.zeros(B, H0, W0, device=DEV), torch.zeros(B, H0, W0, device=DEV)
    ops.blend_paste_stats(*maps, preds[:, :n1], mask, proc[:, :n1], PH, PW)
    ops.blend_paste_frames(avg, cnt, preds[:, :n1], mask, proc[:, :n1], PH, PW)
    ops.blend_update_stats(*maps, preds[:, n1:n1 + n2], mask, proc[:, n1:n1 + n2], PH, PW)
    ops.blend_update_frames(avg, cnt, preds[:, n1:n1 + n2], mask, proc[:, n1:n1 + n2], PH, PW)
    maps = list(ops.blend_resize_stats(*maps, OH, OW))
    avg, cnt = ops.blend_resize(avg, cnt, OH, OW)
    ops.blend_update_stats(*maps, preds[:, n1 + n2:], mask_r, proc[:, n1 + n2:], RH, RW)
    ops.blend_update_frames(avg, cnt, preds[:, n1 + n2:], mask_r, proc[:, n1 + n2:], RH, RW)
    assert torch.equal(maps[0], avg) and torch.equal(maps[1], cnt)
    unc = ops.blend_uncertainty(maps[1], maps[2])
    for f in range(B):
        one = [torch.zeros(H0, W0, device=DEV) for _ in range(4)]
        pr, pt = preds[f], proc[f]
        ops.blend_paste_stats(*one, pr[:n1], mask, pt[:n1].contiguous(), PH, PW)
        ops.blend_update_stats(*one, pr[n1:n1 + n2], mask, pt[n1:n1 + n2].contiguous(), PH, PW)
        one = list(ops.blend_resize_stats(*one, OH, OW))
        ops.blend_update_stats(*one, pr[n1 + n2:], mask_r, pt[n1 + n2:].contiguous(), RH, RW)
        for k in range(4):
            assert torch.equal(maps[k][f], one[k]), (f, k)
        ref = _ref_frame(f, mask, mask_r, preds, rnd, (n1, n2, n3))
        assert np.array_equal(maps[3][f].cpu().numpy(), ref.n)
        _check_u(unc[f].cpu(), ref, float(avg[f].abs().max()))


# ------------------------------------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------------------------------------
def _build(kind, c, sd, **extra):
    from patchrefinerv2_amd import models  # noqa: F401
    from patchrefinerv2_amd.registry import build_model
    cfg = dict(c["ref_config"])
    cfg["coarse_branch"] = dict(type="DA2", pretrained=None, model_cfg={**c["da2_cfg"]})
    if kind == "PatchRefiner":
        cfg["refiner"] = dict(cfg["refiner"])
        cfg["refiner"]["fine_branch"] = dict(type="DA2", pretrained=None, model_cfg={**c["da2_cfg"]})
    cfg.update(extra)
    m = build_model(dict(type=kind, config=cfg))
    m.load_state_dict(sd, strict=True)
    return m


def _frames(m, c, seeds):
    hr = torch.cat([rand_image(s, 1, *c["raw"]) for s in seeds]).to(DEV)
    return hr, m.resizer(hr)


def _tc(c):
    return dict(image_raw_shape=c["raw"], patch_split_num=c["split"])


def _call(m, c, mode, hr, lr, seed=621, **kw):
    random.seed(seed)
    return m(mode="infer", cai_mode=mode, process_num=4, tile_cfg=_tc(c), image_lr=lr, image_hr=hr, **kw)


def _host_count(m, plan, tile_cfg):
    """tiles covering each pixel, from the plan alone: the init / grid footprints at the re-ensemble resolution, resampled nearest to the
    raw resolution in an r-mode, plus the random tiles' footprints"""
    tc = m.prepare_tile_cfg(tile_cfg["image_raw_shape"], tile_cfg["patch_split_num"])
    ph, pw = m.patch_process_shape
    rh, rw = tc["patch_raw_shape"]
    n = np.zeros(tc["patch_reensemble_shape"])
    for p in plan:
        if p["kind"] == "random":
            H, W = tc["image_raw_shape"]
            n = n[np.ix_(_nearest(H, n.shape[0]), _nearest(W, n.shape[1]))]
            for h, w in p["raw"]:
                n[h:h + rh, w:w + rw] += 1
        else:
            for h, w in p["proc"]:
                n[h:h + ph, w:w + pw] = 1 if p["kind"] == "init" else n[h:h + ph, w:w + pw] + 1
    return n


def _ref_model(m, hr, lr, plan, tile_cfg):
    """the restatement driven by predict_tiles on the plan's tiles (bf16x3: per-tile predictions do not depend on batching)"""
    from patchrefinerv2_amd.models import blend_mask
    tc = m.prepare_tile_cfg(tile_cfg["image_raw_shape"], tile_cfg["patch_split_num"])
    ph, pw = m.patch_process_shape
    rh, rw = tc["patch_raw_shape"]
    tiles = [t for p in plan for t in p["raw"]]
    preds = m.predict_tiles(lr, hr, tiles, tile_cfg).view(len(tiles), ph, pw).cpu().numpy()
    mask = blend_mask((ph, pw), m.blend_border, 0.0, "cpu").numpy()
    ref = Ref64(*tc["patch_reensemble_shape"])
    o = 0
    for p in plan:
        k = len(p["raw"])
        if p["kind"] == "init":
            ref.paste(preds[o:o + k], mask, p["proc"], ph, pw)
        elif p["kind"] == "grid":
            ref.update(preds[o:o + k], mask, p["proc"], ph, pw)
        else:
            ref.resize(*tc["image_raw_shape"])
            ref.update(preds[o:o + k], blend_mask((rh, rw), m.blend_border, 1e-3, "cpu").numpy(), p["raw"], rh, rw)
        o += k
    return ref


def _check_model(m, c, mode, seed=621, frame_seed=0):
    hr, lr = _frames(m, c, (frame_seed,))
    d0, _ = _call(m, c, mode, hr, lr, seed)
    d, log = _call(m, c, mode, hr, lr, seed, return_uncertainty=True)
    assert torch.equal(d, d0), mode  # the statistics leave the depth bit-identical
    u, cm = log["uncertainty"], log["count_map"]
    assert u.shape == cm.shape == d.shape and u.dtype == cm.dtype == torch.float32 and not u.is_cuda and not cm.is_cuda
    plan = m.last_plan
    count = _host_count(m, plan, _tc(c))
    assert np.array_equal(cm[0, 0].numpy(), count), mode
    ref = _ref_model(m, hr, lr, plan, _tc(c))
    assert np.array_equal(ref.n, count)
    a_scale = float(d.abs().max())
    assert float(np.abs(ref.a - d[0, 0].numpy()).max()) <= 1e-5 * a_scale  # the predictions the restatement blends are the frame's
    u64 = _check_u(u[0, 0].numpy(), ref, a_scale)
    if mode == "m1":
        assert float(u.abs().max()) == 0.0 and bool((cm == 1).all())
    else:
        assert u64.max() > 0 and int(count.max()) >= 2
    # on the device with return_device=True, same values
    dd, logd = _call(m, c, mode, hr, lr, seed, return_uncertainty=True, return_device=True)
    assert logd["uncertainty"].is_cuda and logd["count_map"].is_cuda
    assert torch.equal(dd.cpu(), d) and torch.equal(logd["uncertainty"].cpu(), u) and torch.equal(logd["count_map"].cpu(), cm)


@pytest.mark.parametrize("mode", ["m1", "m2", "r4", "r12"])
def test_v2_uncertainty_against_float64(mode):
    _check_model(_build("PatchRefinerPlus", E2E_V2, e2e_v2_sd(), prec="bf16x3", max_batch=3, n_streams=2), E2E_V2, mode)


@pytest.mark.parametrize("mode", ["m1", "m2", "r8"])
def test_v1_uncertainty_against_float64(mode):
    _check_model(_build("PatchRefiner", E2E_V1, e2e_v1_sd(), prec="bf16x3", max_batch=3), E2E_V1, mode, frame_seed=1)


def test_frames_equal_single_calls_with_uncertainty():
    """B = 3 in one call (frame-major tile list, one blend launch per pass step) == three single calls, all three outputs bit for bit"""
    c = E2E_V2
    m = _build("PatchRefinerPlus", c, e2e_v2_sd(), prec="bf16x3", max_batch=5, n_streams=3)
    hr, lr = _frames(m, c, (0, 3, 5))
    seeds = [11, 621, 12]
    for mode in ("m2", "r8"):
        single = []
        for f in range(3):
            random.seed(seeds[f])
            d, log = m(mode="infer", cai_mode=mode, process_num=4, tile_cfg=_tc(c), image_lr=lr[f:f + 1], image_hr=hr[f:f + 1],
                       return_uncertainty=True)
            single.append((d, log["uncertainty"], log["count_map"]))
        d, log = m(mode="infer", cai_mode=mode, process_num=4, tile_cfg=_tc(c), image_lr=lr, image_hr=hr, frame_seeds=seeds,
                   return_uncertainty=True)
        assert log["uncertainty"].shape == log["count_map"].shape == d.shape and d.shape[:2] == (3, 1)
        for k, t in enumerate((d, log["uncertainty"], log["count_map"])):
            assert torch.equal(t, torch.cat([s[k] for s in single])), (mode, k)
        for f in range(3):
            assert np.array_equal(log["count_map"][f, 0].numpy(), _host_count(m, m.last_plans[f], _tc(c)))


def test_hip_graph_replay_equals_eager_with_and_without_uncertainty():
    c = E2E_V2
    sd = e2e_v2_sd()
    eager = _build("PatchRefinerPlus", c, sd, prec="bf16x3", max_batch=3, n_streams=2)
    graph = _build("PatchRefinerPlus", c, sd, prec="bf16x3", max_batch=3, n_streams=2, hip_graph=True)
    hr, lr = _frames(eager, c, (2,))
    for it in range(3):  # per key: eager first call, captured second, replayed third -- the two keys in alternation
        for stats in (True, False):
            want = _call(eager, c, "r8", hr, lr, 621 + it, return_uncertainty=stats, return_device=True)
            got = _call(graph, c, "r8", hr, lr, 621 + it, return_uncertainty=stats, return_device=True)
            assert torch.equal(got[0], want[0]), (it, stats)
            if stats:
                for k in ("uncertainty", "count_map"):
                    assert torch.equal(got[1][k], want[1][k]), (it, k)
            else:
                assert "uncertainty" not in got[1] and "count_map" not in got[1]
    graphs = [v for v in graph._graphs.values() if isinstance(v, dict)]
    assert len(graphs) == 2 and sorted(g["stats"] is not None for g in graphs) == [False, True]
    # returned maps are copies: the next replay does not rewrite them
    _, l1 = _call(graph, c, "r8", hr, lr, 5, return_uncertainty=True, return_device=True)
    keep = l1["uncertainty"].clone()
    _call(graph, c, "r8", hr, lr, 6, return_uncertainty=True, return_device=True)
    assert torch.equal(l1["uncertainty"], keep)


def test_f16f6_runs_with_uncertainty():
    from patchrefinerv2_amd import ops
    c = E2E_V2
    m = _build("PatchRefinerPlus", c, e2e_v2_sd(), prec="f16f6", max_batch=4, n_streams=2)
    hr, lr = _frames(m, c, (0, 1))
    for B in (1, 2):
        d0, _ = _call(m, c, "r4", hr[:B], lr[:B], frame_seeds=[7, 8][:B] if B > 1 else None)
        d, log = _call(m, c, "r4", hr[:B], lr[:B], frame_seeds=[7, 8][:B] if B > 1 else None, return_uncertainty=True)
        assert torch.equal(d, d0)
        assert bool(torch.isfinite(log["uncertainty"]).all()) and float(log["uncertainty"].max()) > 0
        assert float(log["count_map"].min()) >= 1
    assert ops.F6Range.active(DEV) and getattr(m, "f6_guarded_frames", 0) > 0


def test_baseline_fine_and_semi_support_uncertainty():
    from oracle.cases import BASELINE, baseline_kwargs, baseline_sd
    from patchrefinerv2_amd import models
    from patchrefinerv2_amd.registry import build_model
    b = build_model(dict(type="BaselinePretrain", **baseline_kwargs("fine"), max_batch=3))
    b.load_dict(baseline_sd())
    hr, lr = _frames(b, BASELINE, (0,))
    d0, log0 = _call(b, BASELINE, "r2", hr, lr)
    d, log = _call(b, BASELINE, "r2", hr, lr, return_uncertainty=True)
    assert log0 == {} and torch.equal(d, d0) and set(log) == {"uncertainty", "count_map"}
    assert np.array_equal(log["count_map"][0, 0].numpy(), _host_count(b, b.last_plan, _tc(BASELINE)))
    c = E2E_V2
    m = _build("PatchRefinerPlus", c, e2e_v2_sd(), prec="bf16x3", max_batch=4)
    semi = object.__new__(models.PatchRefinerSemi)
    semi.__dict__["student_model"] = m
    hr, lr = _frames(m, c, (0,))
    d, log = _call(semi, c, "r4", hr, lr, return_uncertainty=True)
    d1, log1 = _call(m, c, "r4", hr, lr, return_uncertainty=True)
    assert torch.equal(d, d1) and torch.equal(log["uncertainty"], log1["uncertainty"]) and torch.equal(log["count_map"], log1["count_map"])


def test_rejected_uncertainty_modes():
    from oracle.cases import BASELINE, baseline_kwargs, baseline_sd
    from patchrefinerv2_amd.registry import build_model
    c = E2E_V2
    m = _build("PatchRefinerPlus", c, e2e_v2_sd(), prec="bf16x3")
    hr, lr = _frames(m, c, (0,))
    with pytest.raises(ValueError, match="patch-sharded"):
        m(mode="infer", cai_mode="m1", tile_cfg=_tc(c), image_lr=lr, image_hr=hr, shard=(0, 2), return_uncertainty=True)
    b = build_model(dict(type="BaselinePretrain", **baseline_kwargs("coarse")))
    b.load_dict(baseline_sd())
    hr, lr = _frames(b, BASELINE, (0,))
    with pytest.raises(ValueError, match="coarse"):
        b(mode="infer", image_lr=lr, image_hr=hr, return_uncertainty=True)
    d, log = b(mode="infer", image_lr=lr, image_hr=hr)  # (unchanged without the flag)
    assert "uncertainty" not in log and math.prod(d.shape) > 0


# ------------------------------------------------------------------------------------------------------------------------------
# CLI
# ------------------------------------------------------------------------------------------------------------------------------
def test_cli_generate_pl_writes_pseudo_labels(tmp_path):
    from PIL import Image
    (tmp_path / "imgs").mkdir()
    for i in range(2):
        np.save(str(tmp_path / "imgs" / f"frame{i}.npy"), np.random.RandomState(20 + i).rand(90, 160, 3).astype(np.float32))
    cfg = tmp_path / "cfg.py"
    cfg.write_text(f"_base_ = ['{os.path.join(ROOT, 'configs', 'v2_dav2_mobile_u4k.py')}']\n"
                   "model = dict(config=dict(patch_process_shape=[112, 224], image_raw_shape=[256, 512], patch_split_num=[2, 2],\n"
                   "    coarse_branch=dict(model_cfg=dict(encoder='vits', features=256, out_channels=[48, 96, 192, 384]))))\n")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), str(cfg), "--synthetic-weights", "--cai-mode", "r4",
                        "--cfg-option", f"general_dataloader.dataset.rgb_image_dir={tmp_path / 'imgs'}", "--save", "--work-dir", str(out),
                        "--image-raw-shape", "256", "512", "--patch-split-num", "2", "2", "--generate-pl", "--count-thr", "0.2",
                        "--frame-batch", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "frame0: pseudo label (1, 1, 256, 512)" in r.stdout and "frame1: pseudo label" in r.stdout, r.stdout
    suffixes = (".png", "_uint16.png", "_uncert_uint16.png", "_uncert.png", "_count_uint16.png")
    assert sorted(os.listdir(out)) == sorted(f"frame{i}{s}" for i in range(2) for s in suffixes)
    for i in range(2):
        for s in ("_uint16.png", "_uncert_uint16.png", "_count_uint16.png"):
            a = np.asarray(Image.open(str(out / f"frame{i}{s}")))
            assert a.dtype == np.uint16 and a.shape == (256, 512) and a.max() > 0, s
        u16 = np.asarray(Image.open(str(out / f"frame{i}_uncert_uint16.png")))
        c16 = np.asarray(Image.open(str(out / f"frame{i}_count_uint16.png")))
        assert u16.max() <= 256 and np.all(c16 % 256 == 0) and c16.min() >= 256  # whole tile counts, every pixel covered
        for s in (".png", "_uncert.png"):
            a = np.asarray(Image.open(str(out / f"frame{i}{s}")))
            assert a.dtype == np.uint8 and a.shape == (256, 512, 3) and a.std() > 0, s
