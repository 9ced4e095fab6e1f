"""CPU side of tests/test_narrow_kernels_gpu.py: its tables and float64 references are sound before any kernel runs -- the SAME helper
against an independent formulation, the discrimination of SAME from symmetric padding, the share of outputs the clamp cuts, and the
expected kernel of every case against a restatement of the dispatch predicates of csrc/pointwise.hip and csrc/igemm.hip.  Nothing here
loads the library."""
import pytest
import torch
import torch.nn.functional as F

import test_narrow_kernels_gpu as G


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("s", [1, 2])
def test_same_pads_is_tensorflow_same(k, s):
    """an independent statement: the output is ceil(size / s) wide, output o reads inputs o s - low .. o s - low + k - 1, the pads are as
    small as that allows and the odd pixel goes to the high side"""
    for size in range(1, 40):
        low, high = G.same_pads(size, k, s)
        o = -(-size // s)
        assert low >= 0 and high in (low, low + 1)
        assert (size + low + high - k) // s + 1 == o
        assert (o - 1) * s - low + k - 1 - (size - 1) == high    # the last tap of the last output: ``high`` pixels past the image
        if s == 1:
            assert (low, high) == (k // 2, k // 2)
    x = G.rnd(1, 1, 2, 18, 25).double()
    w = G.rnd(2, 2, 2, k, k).double()
    y = G.conv_same64(x, w, None, k, s)
    assert y.shape[2:] == (-(-18 // s), -(-25 // s))
    # every output pixel is the plain correlation at its window, zeros outside the image
    (ly, _), (lx, _) = G.same_pads(18, k, s), G.same_pads(25, k, s)
    big = F.pad(x, (k, k, k, k))
    for oy, ox in ((0, 0), (y.shape[2] - 1, y.shape[3] - 1), (1, 2)):
        win = big[0, :, oy * s - ly + k:oy * s - ly + 2 * k, ox * s - lx + k:ox * s - lx + 2 * k]
        assert torch.allclose(y[0, :, oy, ox], (w * win[None]).sum((1, 2, 3)), rtol=0, atol=1e-12)


def test_stated_pads_of_the_cases():
    assert (G.same_pads(18, 3, 2), G.same_pads(25, 3, 2)) == ((0, 1), (1, 1))      # pad_y 0, pad_x 1
    assert (G.same_pads(35, 5, 2), G.same_pads(18, 5, 2)) == ((2, 2), (1, 2))      # pad_y 2, pad_x 1, high side 2
    assert (G.same_pads(129, 3, 2), G.same_pads(128, 3, 2)) == ((1, 1), (0, 1))    # pad_y 1, pad_x 0
    assert (G.same_pads(130, 3, 2), G.same_pads(127, 3, 2)) == ((0, 1), (1, 1))    # pad_y 0, pad_x 1


def _dw_strip(case):
    """prv2_dwconv2d_ex: stride 1, at least one strip, and the last strip of a row wastes <= 1/8 of the work"""
    n, h, w, c, k, s = case[:6]
    return s == 1 and w >= 8 and ((w + 7) // 8 * 8 - w) * 8 <= w


@pytest.mark.parametrize("case", G.DW_CASES + G.DW_SLICE_CASES + G.DW_OUT_SLICE_CASES[:1], ids=G.dw_id)
def test_depthwise_case(case):
    n, h, w, c, k, s, act, same, bias, kernel = case
    assert c % 4 == 0 and k in (3, 5, 7) and s in (1, 2)
    assert kernel == ("strip" if _dw_strip(case) else "naive")
    ref = G.dw_ref(case)    # (asserts the discrimination of a SAME case itself)
    oh, ow = (-(-h // s), -(-w // s)) if same else ((h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1)
    assert ref.shape == (n, c, oh, ow) and ref.dtype == torch.float32 and bool(torch.isfinite(ref).all())


def test_depthwise_cases_take_the_paths_they_name():
    ids = [G.dw_id(c) for c in G.DW_CASES]
    assert len(set(ids)) == len(ids)
    # a SAME stride-2 case with pad_y != pad_x and one whose low side differs from its high side
    assert any(c[7] and G.same_pads(c[1], c[4], c[5])[0] != G.same_pads(c[2], c[4], c[5])[0] for c in G.DW_CASES)
    assert any(c[7] and G.same_pads(c[2], c[4], c[5])[0] != G.same_pads(c[2], c[4], c[5])[1] for c in G.DW_CASES)
    # a strip case whose last strip has one live pixel, one with exactly one strip, one image of one pixel
    assert any(_dw_strip(c) and c[2] % 8 == 1 for c in G.DW_CASES) and any(_dw_strip(c) and c[2] == 8 for c in G.DW_CASES)
    assert any(c[1] == c[2] == 1 for c in G.DW_CASES)
    assert {c[9] for c in G.DW_SLICE_CASES} == {"strip", "naive"} == {c[9] for c in G.DW_OUT_SLICE_CASES}
    assert any(_dw_strip(c) and c[2] % 8 for c in G.DW_OUT_SLICE_CASES) and all(c[0] == 1 for c in G.DW_OUT_SLICE_CASES)


@pytest.mark.parametrize("case", G.C1_CASES, ids=G.c1_id)
def test_one_output_case(case):
    n, h, w, cin, k, o = case
    assert k in (1, 3) and set(o) <= {"bias", "act", "scale", "res", "layout"}
    ref, share = G.c1_ref(case)   # (asserts 25 % <= share <= 75 % where the clamp is used)
    assert ref.shape == (n, 1, h, w) and (share is not None) == bool(o.get("res"))
    assert G.c1_kernel_name(case) == ("conv_cout1_k3_kernel<32,f32>" if k == 3 else "conv_cout1_k1_kernel<0,f32>")


def test_one_output_cases_take_the_paths_they_name():
    k3 = [c for c in G.C1_CASES if c[4] == 3]
    k1 = [c for c in G.C1_CASES if c[4] == 1]
    assert {c[3] % 4 for c in k3} == {0, 1, 2, 3}                                   # every length of the partial-slab tail
    assert any(c[3] < 32 for c in k3) and any(c[3] > 64 and c[3] % 32 for c in k3)  # under one slab; several slabs, the last partial
    assert any(c[2] > 32 and c[1] > 8 for c in k3) and any(c[1] % 8 == 0 and c[2] % 32 == 0 for c in k3)   # ragged and exact tiles
    assert any(c[3] % 4 for c in k1) and any(c[3] % 4 == 0 for c in k1)             # scalar and float4 path of the 1x1 kernel
    assert all((c[0] * c[1] * c[2]) % 256 for c in k1)
    for cs in (k3, k1):
        assert any(c[5].get("res") for c in cs) and any(c[5].get("act") == "relu" for c in cs)
        assert any(c[5].get("act") == "sigmoid" and c[5].get("scale", 1.0) != 1.0 for c in cs) and any(c[5].get("layout") == "slice" for c in cs)


def _conv_family(case):
    """prv2_conv2d's order for k > 1, no fused LayerNorm: the 3x3 stride-1 halo kernels (pad 1 -- SAME is pad 1 at stride 1 -- width >= 24,
    height >= 4), then the direct kernel for <= 4 input channels (8 .. 64 outputs, <= 49 taps, >= 4096 outputs per image), then igemm_kernel"""
    n, h, w, cin, cout, k, s, o, _ = case
    oh, ow = G.conv_out_hw(case)
    if k == 3 and s == 1 and w >= 24 and h >= 4:
        return "halo"
    if cin <= 4 and 1 < k * k <= 49 and 8 <= cout <= 64 and oh * ow >= 4096:
        return "few_in"
    return "igemm"


ALL_CONV_CASES = G.FEW_IN_CASES + [G.SWITCH_CASE] + G.GENERIC_SAME_CASES + [G.HALO_SAME_CASE]


@pytest.mark.parametrize("case", ALL_CONV_CASES, ids=G.conv_id)
def test_conv_case(case):
    n, h, w, cin, cout, k, s, o, family = case
    assert family == _conv_family(case)
    assert set(o) <= {"same", "bias", "act", "relu_in", "gamma", "res"}
    ref = G.conv_ref(case)   # (asserts the discrimination of a SAME case itself)
    assert ref.shape == (n, cout, *G.conv_out_hw(case)) and bool(torch.isfinite(ref).all())
    assert G.conv_ref(case) is ref   # computed once, shared by the arithmetic modes


def test_conv_cases_take_the_paths_they_name():
    few = [c for c in G.FEW_IN_CASES if c[8] == "few_in"]
    px = [G.conv_out_hw(c)[0] * G.conv_out_hw(c)[1] for c in few]
    assert min(px) == 4096 and all(p >= 4096 for p in px)
    assert {c[3] for c in few} == {1, 2, 3, 4} and {25, 49} <= {c[5] ** 2 for c in few}
    assert any(c[4] % 8 for c in few) and any(c[4] == 64 for c in few) and any(c[7].get("relu_in") for c in few)
    assert any(c[4] % 8 and c[7].get("gamma") and c[7].get("res") and c[7].get("act") for c in few)
    assert any((c[4] + 7) // 8 == 5 and 256 // 5 == 51 for c in few)
    sw = G.SWITCH_CASE
    assert G.conv_out_hw(sw)[0] * G.conv_out_hw(sw)[1] == 4095 and sw[3] <= 4 and 8 <= sw[4] <= 64 and sw[0] == 3
    # SAME cases with pad_y != pad_x on each of the two loaders
    for cs in (few, G.GENERIC_SAME_CASES):
        assert any(c[7].get("same") and G.same_pads(c[1], c[5], c[6])[0] != G.same_pads(c[2], c[5], c[6])[0] for c in cs)
    assert G.CONV_DISCRIMINATION_TOL * 100 >= max(100 * G.CONV_TOL["f32"], 100 * G.CONV_TOL["bf16x3"], 10 * G.CONV_TOL["bf16"])


def test_layernorm_cases_take_the_paths_they_name():
    """prv2_layernorm: float4 kernels up to c = 2048 (MAXV 1, 2, 4, 8 at 256, 512, 1024, 2048), else scalar; grid = min(ceil(rows / 4), 8192)"""
    maxv = lambda c: None if c % 4 or c > 2048 else next(v for v in (1, 2, 4, 8) if c <= 256 * v)  # noqa: E731
    assert [maxv(c) for c in G.LN_CHANNELS] == [8, 8, None, None, None]
    assert 2052 in G.LN_CHANNELS and 2052 % 4 == 0
    blocks = -(-G.LN_ROWS // 4)
    assert blocks > 8192 and G.LN_ROWS - 4 * 8192 < 4 * 8192 and G.LN_ROWS % 4 != 0
    for c in G.LN_CHANNELS:
        x, w, b = G.ln_inputs(c)
        ref = G.ln_ref(x, w, b, "gelu")
        assert ref.shape == x.shape and bool(torch.isfinite(ref).all())
        want = F.gelu(F.layer_norm(x.double().permute(0, 2, 3, 1), (c,), w.double(), b.double(), 1e-6)).permute(0, 3, 1, 2)
        assert float((ref - want.float()).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
