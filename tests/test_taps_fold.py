"""The 256-column gate kernels gathering their coarse addend themselves (prv2_conv3x3_ln_gate_taps / prv2_conv3x3_ln_gate_f6_taps: the column walk of
csrc/coarse_taps_walk.h in the epilogue of csrc/conv3x3_gate_epi.h) against the SAME kernel fed ``CoarseTaps.gather(...)`` as ``pre``.  Both run one
source text for the walk and add its rows to the C tile at the same place, so the requirement is bit equality (torch.equal), not a tolerance."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
F_ = 256
SCALE = 0.25  # spatial_scale of the boxes: frame pixels -> coarse pixels

# (coarse H, W), (output h, w), knot offsets = output pixel pitch in coarse pixels
SHAPES = {
    "q24x32": ((24, 32), (24, 32), (0.25, 0.25)),
    "h16x32": ((16, 32), (16, 32), (0.5, 0.5)),
    "ragged20x24": ((20, 48), (20, 24), (0.25, 0.5)),  # ragged against the 8 x 16 tile on both axes
}


def _ops():
    from patchrefinerv2_amd import ops
    return ops


def _boxes(shape, which):
    """3 tiles (x1, y1, x2, y2) in frame pixels: two opposite frame corners (clamped knots) and one fractional offset"""
    (H, W), (h, w), (kbh, kbw) = SHAPES[shape]
    bh, bw = kbh * h / SCALE, kbw * w / SCALE          # the box whose ROI bin is exactly the knot spacing
    fh, fw = H / SCALE, W / SCALE
    org = {"tl_br": [(0.0, 0.0), (fw - bw, fh - bh), (0.37 * (fw - bw), 0.61 * (fh - bh))],
           "tr_bl": [(fw - bw, 0.0), (0.0, fh - bh), (0.83 * (fw - bw) + 0.3, 0.19 * (fh - bh) + 0.7)]}[which]
    return torch.tensor([[x, y, x + bw, y + bh] for x, y in org], dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def _unit(shape, frames):
    """the operands of one GatedConvUnit tail over 3 tiles of ``shape`` (made once, never written again): fp32 and X2 ``out``, res, the weights of both
    arithmetic modes, and the tap tables of ``frames`` frames (0: single-frame tables)"""
    P = _ops()
    (H, W), (h, w), kb = SHAPES[shape]
    g = torch.Generator(device=DEV).manual_seed(100 + H + w)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    o32 = P.Feat(rnd(3, h, w, F_))
    ox2 = P.Feat(torch.empty(3, h, w, F_, device=DEV), x2=True)
    ident = torch.zeros(F_, F_, 3, 3, device=DEV)
    ident[torch.arange(F_), torch.arange(F_), 1, 1] = 1.0
    P.conv2d(o32, P.pack_conv(ident, None, pad=1, prec=P.L.PREC_NAMES["bf16x3"]), ox2)  # (identity conv: the X2 writer of the 256-column kernel)
    wt, b = rnd(F_, F_, 3, 3) / 48, rnd(F_) * 0.1
    u = dict(o32=o32, ox2=ox2, res=P.Feat(rnd(3, h, w, F_)), ln=(torch.rand(F_, device=DEV, generator=g) + 0.5, rnd(F_) * 0.1),
             gw=P.pack_gate(rnd(F_, F_, 1, 1) / 16), gb=rnd(F_) * 0.1, cw6=P.pack_conv3x3_f6(wt, b),
             cwb=P.pack_conv(wt, b, pad=1, prec=P.L.PREC_NAMES["bf16x3"]))
    u["taps"] = P.CoarseTaps(P.Feat(rnd(max(frames, 1), H, W, 9 * F_) * 0.2), F_, kb)
    torch.cuda.synchronize()
    return u


def _tail(P, u, kernel, x2, with_res, **addend):
    x = u["ox2"] if x2 else u["o32"]
    kw = dict(act=P.ACT_RELU, mul=x, res=u["res"] if with_res else None, pre_cin=F_, **addend)
    if kernel == "f6":
        y = P.conv3x3_ln_gate_f6(x, u["cw6"], u["ln"], u["gw"], u["gb"], **kw)
    else:
        y = P.conv3x3_ln_gate(x, u["cwb"], u["ln"], u["gw"], u["gb"], **kw)
    name = P.L.load().prv2_last_kernel().decode()
    assert name.startswith({"f6": "conv3x3_c256_gate_f6_kernel", "bf16x3": "conv3x3_c256_gate_x2_kernel" if x2 else "conv3x3_c256_gate_kernel"}[kernel]), name
    return y.buf


def _check(P, u, boxes, shape, kernel, x2, with_res):
    (_, _), (h, w), _ = SHAPES[shape]
    folded = _tail(P, u, kernel, x2, with_res, taps=u["taps"], boxes=boxes, spatial_scale=SCALE)
    pre = u["taps"].gather(boxes, SCALE, h, w)
    ref = _tail(P, u, kernel, x2, with_res, pre=pre)
    bare = _tail(P, u, kernel, x2, with_res)
    assert bool(torch.isfinite(ref).all()) and not torch.equal(ref, bare)  # (the addend matters: neither call may have dropped it)
    diff = folded != ref
    assert torch.equal(folded, ref), (int(diff.sum()), diff.nonzero()[:8].tolist(), float((folded - ref).abs().max()))


@pytest.mark.parametrize("x2", [False, True], ids=["fp32", "x2"])
@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("kernel", ["f6", "bf16x3"])
@pytest.mark.parametrize("which", ["tl_br", "tr_bl"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_folded_gather_equals_gathered_pre(shape, which, kernel, with_res, x2):
    """single-frame tables, 4-column boxes in the frame's corners and at fractional offsets"""
    P = _ops()
    _check(P, _unit(shape, 0), _boxes(shape, which), shape, kernel, x2, with_res)


@pytest.mark.parametrize("dispatch", ["torch", "ctypes"])
@pytest.mark.parametrize("kernel", ["f6", "bf16x3"])
def test_folded_gather_two_frames(kernel, dispatch, monkeypatch):
    """tables of two frames and boxes (frame, x1, y1, x2, y2): tile i reads its own frame's tables (batched multi-frame inference), on both
    call routes of the host mirror"""
    P = _ops()
    monkeypatch.setattr(P, "DISPATCH", dispatch)
    shape = "ragged20x24"
    u = _unit(shape, 2)
    b4 = _boxes(shape, "tl_br")
    frame = torch.tensor([[1.0], [0.0], [1.0]], device=DEV)
    boxes = torch.cat([frame, b4], 1).contiguous()
    _check(P, u, boxes, shape, kernel, True, True)
    # the frame index is used: the same tiles on the other frame's tables give something else
    other = torch.cat([1.0 - frame, b4], 1).contiguous()
    a = _tail(P, u, kernel, True, True, taps=u["taps"], boxes=boxes, spatial_scale=SCALE)
    c = _tail(P, u, kernel, True, True, taps=u["taps"], boxes=other, spatial_scale=SCALE)
    assert not torch.equal(a, c)
