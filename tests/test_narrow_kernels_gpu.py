"""GPU parity of the narrow kernels every refiner encoder and every depth head runs -- depthwise (strip / naive), the one-output
convs, conv2d with timm Conv2dSame / TensorFlow "SAME" padding and <= 4 input channels, the wide and the scalar LayerNorm -- against
plain torch in float64 on the CPU, at the smallest shapes that still take each launch path.  The tables and the reference side need
no GPU and no library: tests/test_narrow_kernels_host.py checks them (SAME helper, discrimination, clamp share, expected kernels
against a restatement of the dispatch predicates)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle.fusion import ln_cf  # noqa: E402

DEV = "cuda"
NAN = float("nan")


@pytest.fixture(scope="module")
def P():
    from patchrefinerv2_amd import ops
    ops.L.load()
    return ops


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def close(got, ref, tol, what=""):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = float((got - ref).abs().max())
    scale = max(1.0, float(ref.abs().max()))
    assert err <= tol * scale, f"{what}: max|d|={err:.3e} (scale {scale:.2f})"


def last_kernel(P) -> str:
    return P.L.load().prv2_last_kernel().decode()


def roundup(a, b):
    return (a + b - 1) // b * b


# ---- float64 references --------------------------------------------------------------------------------------------------------

def act64(t, act):
    return {"none": lambda v: v, "relu": F.relu, "gelu": F.gelu, "silu": F.silu, "sigmoid": torch.sigmoid}[act](t)


def act_code(P, act):
    return {"none": P.ACT_NONE, "relu": P.ACT_RELU, "gelu": P.ACT_GELU, "silu": P.ACT_SILU, "sigmoid": P.ACT_SIGMOID}[act]


def same_pads(size, k, s):
    """timm Conv2dSame / TensorFlow "SAME" along one axis -> (low pad, high pad): the output is ceil(size / s), the high side gets the odd pixel"""
    o = -(-size // s)
    total = max((o - 1) * s + k - size, 0)
    return total // 2, total - total // 2


def conv_same64(x, w, b, k, s, groups=1):
    (ly, hy), (lx, hx) = same_pads(x.shape[2], k, s), same_pads(x.shape[3], k, s)
    return F.conv2d(F.pad(x, (lx, hx, ly, hy)), w, b, stride=s, padding=0, groups=groups)


def conv_ref64(x, w, b, k, s, same, tol, groups=1, post=lambda t: t):
    """post(conv) in float64 with SAME or symmetric k // 2 padding.  A SAME case whose low pad differs from k // 2 on some axis must tell
    the two paddings apart: the symmetric result (same output size) has to differ by >= 100 x the case's tolerance -- else the case is void"""
    x, w, b = x.double(), w.double(), (b.double() if b is not None else None)
    if not same:
        return post(F.conv2d(x, w, b, stride=s, padding=k // 2, groups=groups))
    ref = post(conv_same64(x, w, b, k, s, groups))
    if any(same_pads(sz, k, s)[0] != k // 2 for sz in x.shape[2:]):
        sym = post(F.conv2d(x, w, b, stride=s, padding=k // 2, groups=groups))
        if sym.shape == ref.shape:
            d, scale = float((sym - ref).abs().max()), max(1.0, float(ref.abs().max()))
            assert d >= 100 * tol * scale, f"SAME and symmetric padding differ by only {d:.3e} (need {100 * tol * scale:.3e})"
    return ref


# ---- a. depthwise ----------------------------------------------------------------------------------------------------------------
# (n, h, w, c, k, stride, act, same_pad, bias, expected kernel)
DW_CASES = [
    # SAME, stride 2: the naive kernel (pad_y != pad_x, low side != high side)
    (2, 18, 25, 48, 3, 2, "silu", True, True, "naive"),     # pad_y 0, pad_x 1
    (1, 35, 18, 96, 5, 2, "silu", True, True, "naive"),     # pad_y 2, pad_x 1 (high side 2)
    (2, 9, 13, 240, 5, 2, "silu", True, False, "naive"),
    (1, 5, 7, 3072, 3, 2, "silu", True, True, "naive"),
    (1, 12, 10, 32, 7, 2, "none", True, True, "naive"),
    # SAME, stride 1: the strip kernel with bias and activation together
    (1, 9, 31, 64, 5, 1, "silu", True, True, "strip"),
    (2, 6, 57, 32, 7, 1, "relu", True, True, "strip"),      # the last strip has one live pixel
    (1, 4, 8, 16, 3, 1, "gelu", False, True, "strip"),      # exactly one strip per row
    # both sides of the strip predicate
    (1, 5, 9, 32, 7, 1, "none", False, True, "naive"),      # waste 7 * 8 = 56 > 9
    (3, 1, 1, 8, 7, 1, "relu", False, True, "naive"),
    (1, 1, 64, 8, 7, 1, "none", False, False, "strip"),     # every row tap but one out of the image
    # symmetric stride 2 on odd sizes
    (2, 21, 23, 32, 3, 2, "relu", False, True, "naive"),
    (2, 21, 23, 32, 5, 2, "relu", False, True, "naive"),
    (2, 21, 23, 32, 7, 2, "relu", False, True, "naive"),
]
# channel-slice input (ldx > c) / output (ldy > c): one strip shape, one stride-2 (naive) shape
DW_SLICE_CASES = [
    (1, 6, 24, 32, 5, 1, "none", False, True, "strip"),
    (1, 10, 12, 32, 3, 2, "none", False, True, "naive"),
]
# channel-slice output: a strip shape whose last strip is partial (7 live pixels), and the stride-2 shape
DW_OUT_SLICE_CASES = [
    (1, 6, 31, 32, 5, 1, "none", False, True, "strip"),
    (1, 10, 12, 32, 3, 2, "none", False, True, "naive"),
]
DW_TOL = 1e-5


def dw_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-k{c[4]}s{c[5]}-{c[6]}{'-same' if c[7] else ''}{'-bias' if c[8] else ''}"


def dw_kernel_name(case):
    return f"dwconv_{'strip_' if case[9] == 'strip' else ''}kernel<{case[4]},f32>"


def dw_inputs(case):
    n, h, w, c, k = case[:5]
    return rnd(11, n, c, h, w), rnd(12, c, 1, k, k) / k, (rnd(13, c) if case[8] else None)


@functools.lru_cache(maxsize=None)
def dw_ref(case):
    n, h, w, c, k, s, act, same, _, _ = case
    x, wd, b = dw_inputs(case)
    return conv_ref64(x, wd, b, k, s, same, DW_TOL, groups=c, post=lambda t: act64(t, act)).float()


def dw_device_args(case):
    x, wd, b = dw_inputs(case)
    c, k = case[3], case[4]
    return x, wd.view(c, k * k).t().contiguous().to(DEV), (b.to(DEV) if b is not None else None)  # weights tap-major [k*k, C]


def slice_feat(P, x, c0, ld, fill=NAN):
    """x [n, c, h, w] as the channels [c0, c0 + c) of an ld-channel NHWC buffer whose other channels hold ``fill``"""
    n, c, h, w = x.shape
    buf = torch.full((n, h, w, ld), fill, device=DEV)
    buf[..., c0:c0 + c] = x.permute(0, 2, 3, 1).to(DEV)
    return P.Feat(buf).slice(c0, c)


@pytest.mark.parametrize("case", DW_CASES, ids=dw_id)
def test_dwconv2d(P, case):
    n, h, w, c, k, s, act, same, _, _ = case
    x, wt, b = dw_device_args(case)
    y = P.dwconv2d(P.Feat.from_nchw(x.to(DEV)), wt, b, k, s, act=act_code(P, act), same_pad=same)
    assert last_kernel(P) == dw_kernel_name(case), last_kernel(P)
    close(y.to_nchw(), dw_ref(case), DW_TOL, f"dw {dw_id(case)}")


@pytest.mark.parametrize("case", DW_SLICE_CASES, ids=dw_id)
def test_dwconv2d_reads_a_channel_slice(P, case):
    """ldx > c: the input is channels [8, 40) of a 48-channel buffer whose other 16 channels are NaN"""
    n, h, w, c, k, s, act, same, _, _ = case
    x, wt, b = dw_device_args(case)
    y = P.dwconv2d(slice_feat(P, x, 8, 48), wt, b, k, s, act=act_code(P, act), same_pad=same)
    assert last_kernel(P) == dw_kernel_name(case), last_kernel(P)
    close(y.to_nchw(), dw_ref(case), DW_TOL, f"dw slice in {dw_id(case)}")


@pytest.mark.parametrize("case", DW_OUT_SLICE_CASES, ids=dw_id)
def test_dwconv2d_writes_a_channel_slice(P, case):
    """ldy > c: the entry point itself (ops.dwconv2d always allocates a dense output) writes channels [4, 36) of a NaN-filled 40-channel
    buffer; the other 8 channels stay NaN, and so does a guard row of pixels behind the image (a store one pixel past a row's end lands
    in the next row, where the right value may overwrite it -- behind the last row it lands in the guard)"""
    n, h, w, c, k, s, act, same, _, _ = case
    assert n == 1   # (the guard row is contiguous with the one image)
    x, wt, b = dw_device_args(case)
    xf = P.Feat.from_nchw(x.to(DEV))
    ref = dw_ref(case)
    oh, ow = ref.shape[2:]
    out = torch.full((n, oh + 1, ow, 40), NAN, device=DEV)
    P.L.check(P.L.load().prv2_dwconv2d_ex(xf.ptr, n, h, w, c, xf.ld, wt.data_ptr(), b.data_ptr(), k, s, act_code(P, act), int(same),
                                          out.data_ptr() + 16, 40, torch.cuda.current_stream().cuda_stream), "dwconv2d")
    assert last_kernel(P) == dw_kernel_name(case), last_kernel(P)
    got = out.cpu()
    assert bool(torch.isnan(got[:, oh]).all()), "the kernel wrote behind the image"
    got = got[:, :oh]
    close(got[..., 4:36].permute(0, 3, 1, 2), ref, DW_TOL, f"dw slice out {dw_id(case)}")
    assert bool(torch.isnan(got[..., :4]).all()) and bool(torch.isnan(got[..., 36:]).all())


# ---- b. one-output conv ------------------------------------------------------------------------------------------------------------
# (n, h, w, cin, k, opts): bias / act / scale / res (+ clamp0) / layout -- "pad": pad channels up to ld = roundup(cin, 4) hold 1e3,
# "slice": channels [4, 4 + cin) of a (cin + 8)-channel buffer that is NaN elsewhere
C1_CASES = [
    # k = 3: the partial-slab tail (c + 4 > Cin) and several slabs; 9 x 33 = two tile rows, a second tile column one pixel wide
    (2, 9, 33, 8, 3, dict(bias=True)),      # under one slab
    (2, 9, 33, 33, 3, dict(bias=True)),     # ld 36: a one-channel tail
    (2, 9, 33, 34, 3, dict(bias=True)),
    (2, 9, 33, 35, 3, dict(bias=True)),
    (2, 9, 33, 64, 3, dict(bias=True)),     # two full slabs
    (2, 9, 33, 98, 3, dict(bias=True)),     # ld 100: four slabs, the last partial
    # k = 3: exact tiles, epilogues, slice input
    (1, 8, 32, 32, 3, dict()),
    (1, 16, 64, 32, 3, dict()),
    (2, 9, 33, 34, 3, dict(bias=True, act="sigmoid", scale=80.0)),
    (2, 9, 33, 34, 3, dict(bias=True, act="relu")),
    (2, 9, 33, 34, 3, dict(res=True)),
    (2, 9, 33, 32, 3, dict(bias=True, layout="slice")),
    # k = 1: n h w = 2 * 7 * 19 = 266 (not a multiple of 256); Cin % 4 != 0 is the scalar path
    (2, 7, 19, 34, 1, dict(bias=True, act="relu")),
    (2, 7, 19, 3, 1, dict(bias=True, act="sigmoid", scale=80.0)),   # ld 4
    (2, 7, 19, 80, 1, dict(res=True)),
    (2, 7, 19, 32, 1, dict(bias=True)),
    (2, 7, 19, 32, 1, dict(bias=True, act="sigmoid", scale=80.0, layout="slice")),
]
C1_TOL = 1e-5


def c1_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to1-k{c[4]}" + "".join(f"-{k}" if v is True else f"-{v}" for k, v in c[5].items())


def c1_kernel_name(case):
    return "conv_cout1_k3_kernel<32,f32>" if case[4] == 3 else "conv_cout1_k1_kernel<0,f32>"


def c1_inputs(case):
    n, h, w, cin, k, o = case
    return (rnd(31, n, cin, h, w), rnd(32, 1, cin, k, k) / math.sqrt(cin * k * k), (rnd(33, 1) if o.get("bias") else None),
            (rnd(34, n, 1, h, w) if o.get("res") else None))


def c1_ref(case):
    """-> (reference, share of outputs that are negative before the clamp)"""
    n, h, w, cin, k, o = case
    x, wt, b, res = c1_inputs(case)
    y = act64(F.conv2d(x.double(), wt.double(), b.double() if b is not None else None, padding=k // 2), o.get("act", "none")) * o.get("scale", 1.0)
    if res is None:
        return y.float(), None
    y = y + res.double()
    share = float((y < 0).double().mean())
    assert 0.25 <= share <= 0.75, f"clamp0 is not exercised: {share:.2f} of the outputs are negative before it"
    return y.clamp(min=0).float(), share


@pytest.mark.parametrize("case", C1_CASES, ids=c1_id)
def test_conv2d_cout1(P, case):
    n, h, w, cin, k, o = case
    x, wt, b, res = c1_inputs(case)
    xf = slice_feat(P, x, 4, cin + 8) if o.get("layout") == "slice" else slice_feat(P, x, 0, roundup(cin, 4), fill=1e3)
    y = P.conv2d_cout1(xf, wt.to(DEV), b.to(DEV) if b is not None else None, k, act=act_code(P, o.get("act", "none")), scale=o.get("scale", 1.0),
                       res=res.to(DEV) if res is not None else None, clamp0=res is not None)
    assert last_kernel(P) == c1_kernel_name(case), last_kernel(P)
    close(y, c1_ref(case)[0], C1_TOL, f"cout1 {c1_id(case)}")


# ---- c. conv2d: SAME padding, <= 4 input channels -----------------------------------------------------------------------------------
# (n, h, w, cin, cout, k, stride, opts, expected kernel family)
FEW_IN_CASES = [
    (2, 129, 128, 3, 24, 3, 2, dict(same=True, bias=True, act="silu"), "few_in"),  # 65 x 64 = 4160 outputs, pad_y 1, pad_x 0
    (1, 130, 127, 4, 40, 3, 2, dict(same=True, bias=True), "few_in"),              # pad_y 0, pad_x 1; five output groups, 51 pixels per block
    (1, 128, 130, 1, 12, 5, 2, dict(same=True), "few_in"),                         # 25 taps, Cin 1, the last group's second half invalid
    (1, 64, 64, 2, 64, 7, 1, dict(bias=True, relu_in=True, res=True), "few_in"),   # 49 taps, exactly 4096 outputs, eight groups
    # cout % 8 != 0 with the full epilogue.  3 x 3, stride 1, pad 1 at width >= 24 belongs to the halo kernels whatever the channel count
    # (prv2_conv2d asks them first), so the 72 x 60 map of this shape is NOT a conv_few_in_kernel case; the 5 x 5 layer below it is
    # the same map, channels and epilogue on conv_few_in_kernel
    (1, 72, 60, 4, 20, 3, 1, dict(bias=True, act="gelu", gamma=True, res=True), "halo"),
    (1, 72, 60, 4, 20, 5, 1, dict(bias=True, act="gelu", gamma=True, res=True), "few_in"),
]
SWITCH_CASE = (3, 63, 65, 4, 32, 3, 1, dict(bias=True), "halo")   # 4095 outputs per image: the other side of conv_few_in_kernel's switch
GENERIC_SAME_CASES = [
    (2, 18, 25, 48, 96, 3, 2, dict(same=True, bias=True, act="silu"), "igemm"),
    (1, 35, 18, 34, 40, 3, 2, dict(same=True, bias=True), "igemm"),
    (1, 9, 13, 64, 130, 5, 2, dict(same=True), "igemm"),
]
HALO_SAME_CASE = (1, 12, 40, 64, 64, 3, 1, dict(same=True), "halo")
CONV_TOL = {"f32": 2e-5, "bf16x3": 3e-5, "bf16": 2e-2}
# What conv_ref64 is asked for: 100 x the tolerance of the parity-grade modes a case runs in (f32, bf16x3: 3e-5).  For the plain-bf16 run
# 100 x 2e-2 = 2 max|ref| is the largest difference two maps bounded by max|ref| can have at all, so no case could meet it: that run
# is given a factor of 10 (0.2 max|ref|), which is the stricter of the two demands and the one applied to every conv case.
CONV_DISCRIMINATION_TOL = max(CONV_TOL["bf16x3"], CONV_TOL["bf16"] / 10)


def conv_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}-k{c[5]}s{c[6]}" + "".join(f"-{k}" if v is True else f"-{v}" for k, v in c[7].items())


def conv_out_hw(case):
    n, h, w, cin, cout, k, s, o, _ = case
    if o.get("same"):
        return -(-h // s), -(-w // s)
    return (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1


@functools.lru_cache(maxsize=None)
def _conv_inputs(key):
    n, h, w, cin, cout, k, s, oh, ow, bias, gamma, res = key
    return (rnd(21, n, cin, h, w), rnd(22, cout, cin, k, k) / math.sqrt(cin * k * k), rnd(23, cout) if bias else None,
            rnd(24, cout) if gamma else None, rnd(26, n, cout, oh, ow) if res else None)


def conv_inputs(case):
    n, h, w, cin, cout, k, s, o, _ = case
    return _conv_inputs((n, h, w, cin, cout, k, s, *conv_out_hw(case), bool(o.get("bias")), bool(o.get("gamma")), bool(o.get("res"))))


_CONV_REFS: dict = {}


def conv_ref(case):
    """epilogue order of prv2_conv2d: bias, activation, gamma, residual"""
    key = conv_id(case)
    if key not in _CONV_REFS:
        n, h, w, cin, cout, k, s, o, _ = case
        x, wt, b, gamma, res = conv_inputs(case)

        def post(t):
            t = act64(t, o.get("act", "none"))
            if gamma is not None:
                t = t * gamma.double().view(1, -1, 1, 1)
            return t + res.double() if res is not None else t
        _CONV_REFS[key] = conv_ref64(F.relu(x) if o.get("relu_in") else x, wt, b, k, s, bool(o.get("same")), CONV_DISCRIMINATION_TOL, post=post).float()
    return _CONV_REFS[key]


def run_conv(P, case, prec, images=None, same=None):
    """-> (NCHW result on the device, kernel name); ``images``: only the first so many of the case's batch"""
    n, h, w, cin, cout, k, s, o, _ = case
    x, wt, b, gamma, res = conv_inputs(case)
    if images is not None:
        x, res = x[:images], (res[:images] if res is not None else None)
    cw = P.pack_conv(wt.to(DEV), b.to(DEV) if b is not None else None, stride=s, prec=P.L.PREC_NAMES[prec],
                     same_pad=bool(o.get("same")) if same is None else same)
    y = P.conv2d(P.Feat.from_nchw(x.to(DEV)), cw, relu_in=bool(o.get("relu_in")), act=act_code(P, o.get("act", "none")),
                 gamma=gamma.to(DEV) if gamma is not None else None, res=P.Feat.from_nchw(res.to(DEV)) if res is not None else None)
    name = last_kernel(P)
    return y.to_nchw(), name


def check_kernel_family(name, family, prec):
    if family == "few_in":
        assert name == f"conv_few_in_kernel<64,{prec}>", name
    elif family == "igemm":
        assert name.startswith("igemm_kernel<") and name.endswith(f",{prec}>"), name
    else:
        assert name.startswith("conv3x3_halo") and name.endswith(f",{prec}>"), name


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", FEW_IN_CASES, ids=conv_id)
def test_conv2d_few_input_channels(P, case, prec):
    """conv_few_in_kernel in every arithmetic mode (the bf16 modes decode hi + lo from the swizzled packed row), SAME and symmetric pad"""
    y, name = run_conv(P, case, prec)
    check_kernel_family(name, case[8], prec)
    close(y, conv_ref(case), CONV_TOL[prec], f"conv {conv_id(case)} {prec}")


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_conv2d_below_the_few_input_switch_is_batch_independent(P, prec):
    """4095 outputs per image: not conv_few_in_kernel, whatever the batch -- image 0 of three has the bits of image 0 alone"""
    y3, name3 = run_conv(P, SWITCH_CASE, prec)
    y1, name1 = run_conv(P, SWITCH_CASE, prec, images=1)
    assert "conv_few_in_kernel" not in name3 and name1 == name3, (name1, name3)   # (f32 mode names its last launch: the remainder strip's igemm_kernel)
    close(y3, conv_ref(SWITCH_CASE), CONV_TOL[prec], f"conv {conv_id(SWITCH_CASE)} {prec}")
    assert torch.equal(y3[:1], y1)


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
@pytest.mark.parametrize("case", GENERIC_SAME_CASES, ids=conv_id)
def test_conv2d_same_pad_generic_kernel(P, case, prec):
    """igemm_kernel's loader (a_iy0 / a_ix0) with pad_y != pad_x"""
    y, name = run_conv(P, case, prec)
    check_kernel_family(name, case[8], prec)
    close(y, conv_ref(case), CONV_TOL[prec], f"conv {conv_id(case)} {prec}")


@pytest.mark.parametrize("prec", ["f32", "bf16x3"])
def test_conv2d_same_pad_stride1_is_symmetric_pad_on_the_halo_kernel(P, prec):
    """stride 1: SAME == pad 1, same kernel, bit for bit"""
    ys, ns = run_conv(P, HALO_SAME_CASE, prec)
    yp, np_ = run_conv(P, HALO_SAME_CASE, prec, same=False)
    check_kernel_family(ns, HALO_SAME_CASE[8], prec)
    assert ns == np_, (ns, np_)
    assert torch.equal(ys, yp)
    close(ys, conv_ref(HALO_SAME_CASE), CONV_TOL[prec], f"conv {conv_id(HALO_SAME_CASE)} {prec}")


# ---- d. LayerNorm ------------------------------------------------------------------------------------------------------------------
LN_TOL = 1e-5
LN_CHANNELS = [1536, 2048, 2052, 6, 1]   # layernorm_kernel<8>, its upper edge, the scalar fallback with c % 4 == 0, and with c % 4 != 0
LN_ROWS = 4 * 8192 + 5                    # a grid of 8192 blocks x 4 rows: the grid-stride loop's second trip ends in a partial block


def ln_inputs(c, n=3, h=7, w=5):
    return rnd(41, n, c, h, w) * 3 + 1, rnd(42, c), rnd(43, c)


def ln_ref(x, w, b, act):
    return act64(ln_cf(x.double(), w.double(), b.double()), act).float()


@pytest.mark.parametrize("act", ["none", "gelu"])
@pytest.mark.parametrize("c", LN_CHANNELS)
def test_layernorm_widths(P, c, act):
    x, w, b = ln_inputs(c)
    out = P.layernorm_feat(P.Feat.from_nchw(x.to(DEV)), w.to(DEV), b.to(DEV), 1e-6, act_code(P, act))
    close(out.to_nchw(), ln_ref(x, w, b, act), LN_TOL, f"ln c={c} {act}")


@pytest.mark.parametrize("act", ["none", "gelu"])
def test_layernorm_grid_stride_second_trip(P, act):
    c = 32
    x, w, b = rnd(44, LN_ROWS, c) * 3 + 1, rnd(42, c), rnd(43, c)
    y = torch.full((LN_ROWS, c), NAN, device=DEV)
    P.layernorm_rows(x.to(DEV), LN_ROWS, c, c, w.to(DEV), b.to(DEV), 1e-6, act_code(P, act), y, c)
    ref = ln_ref(x.t().reshape(1, c, LN_ROWS, 1), w, b, act)[0, :, :, 0].t()
    close(y, ref, LN_TOL, f"ln rows={LN_ROWS} {act}")


@pytest.mark.parametrize("act", ["none", "gelu"])
def test_layernorm_slice_to_slice(P, act):
    """ldx > c (NaN neighbours) into ldy > c (neighbours untouched)"""
    c = 32
    x, w, b = ln_inputs(c, 2, 5, 9)
    xf = slice_feat(P, x, 8, 48)
    obuf = torch.full((2, 5, 9, 40), -7.5, device=DEV)
    P.layernorm_feat(xf, w.to(DEV), b.to(DEV), 1e-6, act_code(P, act), out=P.Feat(obuf).slice(4, c))
    got = obuf.cpu()
    close(got[..., 4:36].permute(0, 3, 1, 2), ln_ref(x, w, b, act), LN_TOL, f"ln slice {act}")
    assert bool((got[..., :4] == -7.5).all()) and bool((got[..., 36:] == -7.5).all())
