"""GPU parity of the GatedConvUnit tail kernels -- conv3x3_c256_kernel / conv3x3_c256_gate_kernel / conv3x3_c256_gate_x2_kernel
(csrc/conv3x3_gate.hip, csrc/conv3x3_gate_epi.h), the 32 / 128-column gate variant of csrc/conv3x3_m16.hip -- and of the coarse-tap
tables (csrc/coarse_taps.hip, csrc/coarse_taps_walk.h) against plain float64 on the CPU, at the smallest shapes that still cross every
edge of the tiles, with every operand combination the entry point admits, on channel slices, and on data built so that float64 pins a
numerical property of the epilogue (two-pass statistics, ln_eps, sigmoid_fast on its rails).

    y = mul . sigmoid(W_g . act(LN_eps(conv3x3(relu_in?(x)) + b [+ pre])) + b_g) + res          (gate_w = None: y = act(LN(...)))

What the kernels take as the VALUE of an operand: the X2 kernel reads x and mul as hi + lo of their bf16 split (x2_reconstruct); the
fp32-format 256-column kernel reads mul as hi + lo too; the 32 / 128-column kernels take mul as it is.  The reconstruction of x cannot be
told from x itself at this bar (it moves the operands by 2^-17 of their size, the bar is 2e-5 of the result's), the one of mul is pinned
by the saturation case: there sigmoid is exactly 1 on a quarter of the channels, mul is ~4096 and res = -mul + randn, so y = mul + res
shows the low bits of mul.

bf16 mode: the conv rounds x and its weights to bf16 (the halo loader stores only the hi plane, the main loop reads only the hi half of
the packed weights: ONE product per slab instead of lo*hi, hi*lo, hi*hi); the gate GEMM rounds act(LN(...)) and the gate weights the same
way; accumulation, bias, LayerNorm, sigmoid, mul (hi + lo at 256 columns) and res stay fp32.  tail_emulate_bf16 does exactly these
roundings around float64 arithmetic; a case's bar is 4 x its error (BF16_CASES), never above the project's 2e-2.

The tables, the references and the data conditions need no GPU and no library: tests/test_gate_tail_host.py checks them."""
import collections
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENTINEL = -7.5
TOL = 2e-5        # bf16x3: the bar test_hip_ops.py::test_conv3x3_ln_gate_fused_tail holds these kernels to
UNIT_TOL = 4e-5   # the whole unit: test_hip_ops.py::test_gated_unit_with_coarse_taps_vs_fp32_reference
TAP_TOL = 3e-6    # the tap tables: test_hip_ops.py::test_coarse_tap_gather_is_conv_of_the_roi
BF16_CAP = 2e-2


@pytest.fixture(scope="module")
def P():
    from patchrefinerv2_amd import ops
    ops.L.load()
    return ops


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def share_of(got, ref, tol):
    """max|got - ref| as a share of the bar tol * max(1, |ref|max)"""
    return float((got.double() - ref.double()).abs().max()) / (tol * max(1.0, float(ref.abs().max())))


def close(got, ref, tol, what):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    s = share_of(got, ref, tol)
    print(f"SHARE {what}: {s:.3f} of {tol:g}")
    assert s <= 1.0, f"{what}: max|d| is {s:.3f} of the bar {tol:g} * max(1, |ref|max = {float(ref.abs().max()):.2f})"


def last_kernel(P) -> str:
    return P.L.load().prv2_last_kernel().decode()


# ---- the X2 format on the CPU ----------------------------------------------------------------------------------------------------

def x2_reconstruct(v):
    """what an X2 element stands for: bf16 hi (RNE) + bf16 lo (RNE of the remainder) (test_hip_ops.py::_x2_reconstruct)"""
    hi = v.to(torch.bfloat16).float()
    return hi + (v - hi).to(torch.bfloat16).float()


def x2_pack(v):
    """fp32 [..., c] (c % 8 == 0) -> the float32 CONTAINER of its X2 image: per 8 channels [8 bf16 hi | 8 bf16 lo] (include/prv2.h)"""
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    g = torch.cat([hi.reshape(*v.shape[:-1], -1, 8), lo.reshape(*v.shape[:-1], -1, 8)], -1)
    return g.reshape(*v.shape[:-1], -1).contiguous().view(torch.float32)


def x2_unpack(c):
    g = c.contiguous().view(torch.bfloat16).reshape(*c.shape[:-1], -1, 16).float()
    return (g[..., :8] + g[..., 8:]).reshape(c.shape)


# ---- A. the tail: cases ------------------------------------------------------------------------------------------------------------
# family -> (output channels, x / mul arrive pre-split, mul counts as hi + lo)
FAMILIES = {"c256": (256, False, True), "c256x2": (256, True, True), "n128": (128, False, False), "n32": (32, False, False)}
KERNELS = {"gate": "conv3x3_c256_gate_kernel<256,{}>", "gx2": "conv3x3_c256_gate_x2_kernel<256,{}>", "plain": "conv3x3_c256_kernel<256,{}>",
           "h128": "conv3x3_halo16_gate_kernel<128,{}>", "h32": "conv3x3_halo16_gate_kernel<32,{}>"}
FAMILY_KERNEL = {"c256": "gate", "c256x2": "gx2", "n128": "h128", "n32": "h32"}

# operand rows: what differs from "every operand present, ReLU, ln_eps 1e-6" (wscale: the conv's weights, bias and addend times this, so that
# the variance in front of the LayerNorm is ~1e-2 and ln_eps = 1e-2 halves the normalised values)
ROW_DEFAULTS = dict(bias=True, gate=True, gate_bias=True, mul=True, res=True, pre=False, act="relu", relu_in=False, ln_eps=1e-6, wscale=1.0)
ROWS = {
    "all": dict(),
    "no_bias": dict(bias=False),
    "no_gate_bias": dict(gate_bias=False),
    "no_mul": dict(mul=False),
    "no_res": dict(res=False),
    "act_none": dict(act="none"),
    "relu_in": dict(relu_in=True),
    "plain": dict(gate=False, gate_bias=False, mul=False, res=False),
    "plain_pre": dict(gate=False, gate_bias=False, mul=False, res=False, pre=True),
    "gate_pre": dict(pre=True),
    "ln_eps": dict(ln_eps=1e-2, wscale=0.1),
}
# family -> row -> the kernel the row expects, or "reject": the entry point is documented to refuse it (RuntimeError).
#   X2 input: no input ReLU, and only the gate kernel reads it; 32 / 128 columns: the entry point has no kernel without the gate stage.
#   ``pre`` with the gate at 32 / 128 columns: conv_plan sends every gate layer to ConvHalo::GATE whatever else it carries, ln_gate_impl has
#   checked the addend's layout, and halo16_body adds p.pre to the C tile in front of the GATE branch -- accepted.
OPERAND_TABLE = {
    "c256": {"all": "gate", "no_bias": "gate", "no_gate_bias": "gate", "no_mul": "gate", "no_res": "gate", "act_none": "gate", "relu_in": "gate",
             "plain": "plain", "plain_pre": "plain", "gate_pre": "gate", "ln_eps": "gate"},
    "c256x2": {"all": "gx2", "no_bias": "gx2", "no_gate_bias": "gx2", "no_mul": "gx2", "no_res": "gx2", "act_none": "gx2", "relu_in": "reject",
               "plain": "reject", "plain_pre": "reject", "gate_pre": "gx2", "ln_eps": "gx2"},
    "n128": {"all": "h128", "no_bias": "h128", "no_gate_bias": "h128", "no_mul": "h128", "no_res": "h128", "act_none": "h128", "relu_in": "h128",
             "plain": "reject", "plain_pre": "reject", "gate_pre": "h128", "ln_eps": "h128"},
    "n32": {"all": "h32", "no_bias": "h32", "no_gate_bias": "h32", "no_mul": "h32", "no_res": "h32", "act_none": "h32", "relu_in": "h32",
            "plain": "reject", "plain_pre": "reject", "gate_pre": "h32", "ln_eps": "h32"},
}

# data: "randn" | "offset" (stress 1) | "zero" (stress 2) | "sat" (stress 3) | "concat" (x = the unit's X2 concat buffer, mul = its first half)
Case = collections.namedtuple("Case", "fam n h w cin row data")

# (n, h, w, cin).  256 columns: 8 x 16 tile, 32-channel slabs, three weight buffers
C256_SHAPES = [(1, 1, 16, 32), (3, 3, 16, 96), (1, 8, 16, 64), (3, 9, 17, 128), (1, 7, 31, 512), (1, 8, 32, 32), (3, 13, 33, 64)]
# 128 / 32 columns: 8 x 32 tile, w >= 24, h >= 4, merged remainder strip (32 x 8 tiles) when w % 32 in 1..8 and w >= 64
NARROW_SHAPES = [(1, 4, 24, 32), (3, 5, 25, 96), (1, 8, 32, 256), (3, 9, 33, 32), (1, 8, 65, 96), (1, 9, 72, 256), (3, 5, 73, 32)]
OPS_SHAPE = {"c256": (3, 9, 17, 64), "c256x2": (3, 9, 17, 64), "n128": (3, 9, 72, 32), "n32": (3, 9, 72, 32)}   # ragged; 72 = 2 tiles + a strip of 8
ZERO_BLOCK = (2, 5, 5, 7)  # stress 2: x = 0 on rows [2, 7) x columns [5, 12): the 3 x 5 interior outputs are exactly the bias

SHAPE_CASES = ([Case(f, *s, "all", "randn") for f in ("c256", "c256x2") for s in C256_SHAPES] + [Case("c256", *s, "plain", "randn") for s in C256_SHAPES[:4]] +
               [Case(f, *s, "all", "randn") for f in ("n128", "n32") for s in NARROW_SHAPES])
OPERAND_CASES = [Case(f, *OPS_SHAPE[f], row, "randn") for f in FAMILIES for row in ROWS]
STRESS_CASES = [Case(f, *OPS_SHAPE[f], "ln_eps" if d == "zero" else "all", d) for f in FAMILIES for d in ("offset", "zero", "sat")]
SLICE_CASES = [Case(f, *OPS_SHAPE[f], "gate_pre", "randn") for f in FAMILIES] + [Case("c256x2", 1, 9, 17, 512, "gate_pre", "concat")]
# bf16 mode: (case, error of tail_emulate_bf16 against float64 as a share of max(1, |ref|max), measured on the CPU by the host test)
BF16_CASES = [
    (Case("c256", *OPS_SHAPE["c256"], "all", "randn"), 9.301e-4),
    (Case("c256", *OPS_SHAPE["c256"], "plain", "randn"), 2.199e-3),
    (Case("c256x2", *OPS_SHAPE["c256x2"], "all", "randn"), 9.303e-4),
    (Case("n128", *OPS_SHAPE["n128"], "all", "randn"), 1.005e-3),
    (Case("n32", *OPS_SHAPE["n32"], "all", "randn"), 8.823e-4),
]


def case_id(c):
    return f"{c.fam}-{c.n}x{c.h}x{c.w}-{c.cin}-{c.row}" + ("" if c.data == "randn" else f"-{c.data}")


def row_of(case):
    o = dict(ROW_DEFAULTS, **ROWS[case.row])
    if case.data == "zero":
        o = dict(o, wscale=1.0)   # (the small variance comes from the zero block, not from the weights)
    return o


def expected_kernel(case):
    return OPERAND_TABLE[case.fam][case.row]


def bf16_bar(emu):
    return min(4.0 * emu, BF16_CAP)


# ---- A. the tail: data and float64 reference ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tail_inputs(case):
    """CPU fp32 operands of a case (NCHW), made once and never written again"""
    cout = FAMILIES[case.fam][0]
    o = row_of(case)
    n, h, w, cin, s = case.n, case.h, case.w, case.cin, o["wscale"]
    sd = 1000 * h + 10 * w + cin + cout
    d = dict(x=rnd(sd + 1, n, cin, h, w), w0=rnd(sd + 2, cout, cin, 3, 3) / math.sqrt(9 * cin) * s, b0=rnd(sd + 3, cout) * 0.5 * s,
             lnw=1 + 0.2 * rnd(sd + 4, cout), lnb=0.1 * rnd(sd + 5, cout), w3=rnd(sd + 6, cout, cout) / math.sqrt(cout), b3=rnd(sd + 7, cout) * 0.5,
             mul=rnd(sd + 8, n, cout, h, w), res=rnd(sd + 9, n, cout, h, w), pre=rnd(sd + 10, n, cout, h, w) * 0.5 * s)
    q = cout // 4
    if case.data == "offset":     # a common offset 100 in front of the LayerNorm: one-pass statistics lose 4 digits, two-pass none
        d["b0"] = 100 + 0.1 * rnd(sd + 11, cout)
    elif case.data == "zero":     # zero block: conv = 0, the LayerNorm sees the bias alone (variance 1e-4: ln_eps = 1e-2 against 1e-6 is a factor 10)
        y0, y1, x0, x1 = ZERO_BLOCK[0], ZERO_BLOCK[0] + ZERO_BLOCK[2], ZERO_BLOCK[1], ZERO_BLOCK[1] + ZERO_BLOCK[3]
        d["x"][:, :, y0:y1, x0:x1] = 0.0
        d["b0"] = 0.5 + 1e-2 * rnd(sd + 11, cout)
    elif case.data == "sat":      # gate bias +100 / -100 on a quarter of the channels each; on the +100 quarter y = mul + res shows mul's low bits
        d["b3"][:q] = 100.0
        d["b3"][q:2 * q] = -100.0
        d["mul"][:, :q] = 4096 * (1 + 0.2 * rnd(sd + 12, n, q, h, w))
        d["res"][:, :q] = -d["mul"][:, :q] + rnd(sd + 13, n, q, h, w)
    elif case.data == "concat":
        assert cin == 2 * cout
        d["mul"] = d["x"][:, :cout]
    return d


def conv64(x, w0, relu_in):
    return F.conv2d(F.relu(x.double()) if relu_in else x.double(), w0.double(), None, padding=1)


def ln64(y, lnw, lnb, eps):
    u = y.mean(1, keepdim=True)
    var = (y - u).pow(2).mean(1, keepdim=True)
    return (y - u) / torch.sqrt(var + eps) * lnw.view(1, -1, 1, 1) + lnb.view(1, -1, 1, 1)


def tail_finish(y, d, o, mul, dt=torch.float64, ln=ln64, stats=None):
    """everything behind the conv, in ``dt``: y = conv3x3(x) without bias; ``o``: the row's switches; ``mul``: its VALUE for this family"""
    c = lambda t: t.to(dt)  # noqa: E731
    if o["bias"]:
        y = y + c(d["b0"]).view(1, -1, 1, 1)
    if o["pre"]:
        y = y + c(d["pre"])
    t = ln(y, c(d["lnw"]), c(d["lnb"]), o["ln_eps"])
    if stats is not None:
        stats["cut"] = float((t < 0).double().mean())
    if o["act"] == "relu":
        t = F.relu(t)
    if not o["gate"]:
        return t
    z = torch.einsum("oc,nchw->nohw", c(d["w3"]), t)
    if o["gate_bias"]:
        z = z + c(d["b3"]).view(1, -1, 1, 1)
    if stats is not None:
        stats["z"] = z
    out = torch.sigmoid(z)
    if o["mul"]:
        out = c(mul) * out
    return out + c(d["res"]) if o["res"] else out


def operand_values(case, d):
    """(x, mul) as the family's kernels take them"""
    _, x_x2, mul_x2 = FAMILIES[case.fam]
    return (x2_reconstruct(d["x"]) if x_x2 else d["x"]), (x2_reconstruct(d["mul"]) if mul_x2 else d["mul"])


@functools.lru_cache(maxsize=None)
def tail_conv(case):
    d, o = tail_inputs(case), row_of(case)
    return conv64(operand_values(case, d)[0], d["w0"], o["relu_in"])


@functools.lru_cache(maxsize=None)
def tail_ref(case):
    """-> (float64 reference, statistics of the data: share cut by the ReLU, the gate pre-activations)"""
    d, o = tail_inputs(case), row_of(case)
    stats = {}
    return tail_finish(tail_conv(case), d, o, operand_values(case, d)[1], stats=stats), stats


def bf16r(t):
    return t.float().to(torch.bfloat16).double()


def tail_emulate_bf16(case):
    """the bf16 mode's roundings (head of the file) around float64 arithmetic"""
    d, o = tail_inputs(case), row_of(case)
    x, mul = operand_values(case, d)
    y = F.conv2d(bf16r(F.relu(x) if o["relu_in"] else x), bf16r(d["w0"]), None, padding=1)
    o2 = dict(o, gate=False)
    t = tail_finish(y, d, o2, mul)
    if not o["gate"]:
        return t
    z = torch.einsum("oc,nchw->nohw", bf16r(d["w3"]), bf16r(t))
    if o["gate_bias"]:
        z = z + d["b3"].double().view(1, -1, 1, 1)
    out = torch.sigmoid(z)
    if o["mul"]:
        out = mul.double() * out
    return out + d["res"].double() if o["res"] else out


# ---- A. the tail: on the GPU -------------------------------------------------------------------------------------------------------

def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def feat(P, t, x2=False, sl=None):
    """NCHW CPU tensor -> Feat: dense, or (sl = (c0, ld)) channels [c0, c0 + c) of an ld-channel buffer that is NaN elsewhere; x2: pre-split bytes"""
    v = x2_pack(nhwc(t)) if x2 else nhwc(t)
    if sl is None:
        return P.Feat(v.to(DEV), x2=x2)
    c0, ld = sl
    buf = torch.full((*v.shape[:3], ld), NAN)
    buf[..., c0:c0 + v.shape[3]] = v
    return P.Feat(buf.to(DEV), x2=x2).slice(c0, v.shape[3])


def run_tail(P, case, prec="bf16x3", slices=False):
    """-> (NCHW result on the CPU, kernel name, the whole output buffer)"""
    cout, x_x2, _ = FAMILIES[case.fam]
    d, o = tail_inputs(case), row_of(case)
    PR = P.L.PREC_NAMES[prec]
    cw = P.pack_conv(d["w0"].to(DEV), d["b0"].to(DEV) if o["bias"] else None, pad=1, prec=PR)
    sl = (lambda c0, ld: (c0, ld)) if slices else (lambda c0, ld: None)
    if case.data == "concat":   # the unit's concat buffer [out | coarse ROI], whole, as x; its first half as mul
        x = feat(P, d["x"], x2=True)
        mul = x.slice(0, cout)
    else:
        x = feat(P, d["x"], x2=x_x2, sl=sl(8, case.cin + 16))
        mul = feat(P, d["mul"], x2=x_x2, sl=sl(8, cout + 16)) if o["mul"] else None
    res = feat(P, d["res"], sl=sl(4, cout + 8)) if o["res"] else None
    pre = feat(P, d["pre"], sl=sl(8, cout + 12)) if o["pre"] else None
    out = None
    if slices:
        out = P.Feat(torch.full((case.n, case.h, case.w, cout + 8), SENTINEL, device=DEV)).slice(4, cout)
    y = P.conv3x3_ln_gate(x, cw, (d["lnw"].to(DEV), d["lnb"].to(DEV)), P.pack_gate(d["w3"].to(DEV)) if o["gate"] else None,
                          d["b3"].to(DEV) if o["gate_bias"] else None, out, act=P.ACT_RELU if o["act"] == "relu" else P.ACT_NONE, mul=mul, res=res,
                          relu_in=o["relu_in"], ln_eps=o["ln_eps"], pre=pre, pre_cin=cout if pre is not None else 0)
    name = last_kernel(P)
    buf = y.buf.cpu()
    return buf[..., y.c0:y.c0 + cout].permute(0, 3, 1, 2), name, buf


def check_tail(P, case, prec="bf16x3", tol=TOL, slices=False):
    want = expected_kernel(case)
    if want == "reject":
        with pytest.raises(RuntimeError):
            run_tail(P, case, prec, slices)
        return None
    got, name, buf = run_tail(P, case, prec, slices)
    assert name == KERNELS[want].format(prec), (name, want)
    close(got, tail_ref(case)[0], tol, f"{case_id(case)} {prec}")
    return buf


@pytest.mark.parametrize("case", SHAPE_CASES, ids=case_id)
def test_tail_shapes(P, case):
    """every tile edge of the two tile shapes: h below the tile height, exact tiles, one live column, 1 / 2 / 3 / 4 / 16 slabs, the strip"""
    check_tail(P, case)


@pytest.mark.parametrize("case", OPERAND_CASES, ids=case_id)
def test_tail_operands(P, case):
    """every operand combination the entry point admits (and the RuntimeError of those it is documented to refuse)"""
    check_tail(P, case)


def test_tail_rejects_presplit_operands_at_32_and_128_columns(P):
    for fam in ("n128", "n32"):
        case = Case(fam, *OPS_SHAPE[fam], "all", "randn")
        d = tail_inputs(case)
        cout = FAMILIES[fam][0]
        cw = P.pack_conv(d["w0"].to(DEV), d["b0"].to(DEV), pad=1, prec=P.L.PREC_NAMES["bf16x3"])
        ln, gw = (d["lnw"].to(DEV), d["lnb"].to(DEV)), P.pack_gate(d["w3"].to(DEV))
        for x2x, x2m in ((True, True), (False, True), (True, False)):
            with pytest.raises(RuntimeError):
                P.conv3x3_ln_gate(feat(P, d["x"], x2=x2x), cw, ln, gw, d["b3"].to(DEV), mul=feat(P, d["mul"], x2=x2m), res=feat(P, d["res"]))
        assert cout in (32, 128)


@pytest.mark.parametrize("case", STRESS_CASES, ids=case_id)
def test_tail_stress(P, case):
    """offset: two-pass statistics; zero: ln_eps arrives, zero padding; sat: sigmoid_fast through inf and 0 without a NaN"""
    check_tail(P, case)


@pytest.mark.parametrize("case", SLICE_CASES, ids=case_id)
def test_tail_channel_slices(P, case):
    """x, mul, res, pre and out as channel slices (ld > c, channel offset 4 or 8: 16-byte aligned) of buffers that are NaN outside the input
    slices; the channels beside the output slice come back bit-identical"""
    buf = check_tail(P, case, slices=True)
    cout = FAMILIES[case.fam][0]
    assert bool((buf[..., :4] == SENTINEL).all()) and bool((buf[..., 4 + cout:] == SENTINEL).all())


@pytest.mark.parametrize("case,emu", BF16_CASES, ids=lambda v: case_id(v) if isinstance(v, Case) else f"emu{v:.2e}")
def test_tail_bf16_mode(P, case, emu):
    assert 0 < bf16_bar(emu) <= BF16_CAP
    check_tail(P, case, prec="bf16", tol=bf16_bar(emu))


# ---- B. the tap tables ---------------------------------------------------------------------------------------------------------------
TAP_SCALE = 0.25                      # spatial_scale of the boxes: frame pixels -> coarse pixels
TAP_MAP = (12, 16)                    # coarse H x W
TAP_TILES = [(1, 1), (1, 5), (2, 2), (3, 16), (13, 18)]                     # oh x ow: 1 x 1 hides 8 of 9 taps, at 2 x 2 every pixel is a corner
TAP_KNOTS = [(0.5, 0.5), (1.0 / 3.0, 1.0 / 5.0), (1.0 / 16.0, 1.0 / 4.0)]   # zero-width middle cell / non-dyadic / anisotropic
TapCase = collections.namedtuple("TapCase", "cout frames cin kb tile slices")
TAP_CASES = [TapCase((256, 32)[(i + j) % 2], (1, 2)[(i + 2 * j) % 3 == 0 or (i, j) == (1, 1)], 4 + (3 * i + j) % 5, kb, tile, False)
             for i, kb in enumerate(TAP_KNOTS) for j, tile in enumerate(TAP_TILES)]
TAP_SLICE_CASES = [TapCase(256, 1, 4, TAP_KNOTS[1], (3, 16), True), TapCase(32, 2, 8, TAP_KNOTS[2], (13, 18), True)]


def tap_id(c):
    return f"{c.cout}ch-{c.frames}f-cin{c.cin}-kb{c.kb[0]:.3f}x{c.kb[1]:.3f}-{c.tile[0]}x{c.tile[1]}" + ("-slices" if c.slices else "")


def tap_boxes(case):
    """[k, 5] fp32 (frame, x1, y1, x2, y2): every box spans kb * (oh, ow) / scale frame pixels (ROI bin == knot spacing).  The four frame
    corners (clamped samples and knot cells), two fractional phases, one whose samples start exactly on a knot; frames interleaved, with
    (B = 2) one index below 0 and one >= B, which the kernels clamp"""
    (H, W), (oh, ow), (kbh, kbw) = TAP_MAP, case.tile, case.kb
    bh, bw = kbh * oh / TAP_SCALE, kbw * ow / TAP_SCALE
    fh, fw = H / TAP_SCALE, W / TAP_SCALE
    on_knot = ((0.5 - 0.5 * kbw + 5) / TAP_SCALE, (0.5 - 0.5 * kbh + 3) / TAP_SCALE)   # sample (0, 0) sits on coarse pixel (3, 5)
    org = [(0.0, 0.0), (fw - bw, 0.0), (0.0, fh - bh), (fw - bw, fh - bh), (0.37 * (fw - bw), 0.61 * (fh - bh)),
           (0.83 * (fw - bw) + 0.3, 0.19 * (fh - bh) + 0.7), on_knot]
    frames = [0.0, 1.0, 0.0, 1.0, -1.0, 2.0, 1.0] if case.frames > 1 else [0.0] * 7
    return torch.tensor([[f, x, y, x + bw, y + bh] for f, (x, y) in zip(frames, org)], dtype=torch.float32)


def roi_axis64(v, n):
    """torchvision's clamp rules along one axis (roi_align.h bilinear_interpolate): -> (lo, hi, weight of hi, inside)"""
    inside = (v >= -1.0) & (v <= n)
    v = v.clamp(min=0.0)
    lo = v.floor().long()
    top = lo >= n - 1
    lo = torch.where(top, torch.full_like(lo, n - 1), lo)
    hi = torch.where(top, lo, lo + 1)
    v = torch.where(top, lo.double(), v)
    return lo, hi, v - lo.double(), inside


def roi_align64(feat64, boxes5, oh, ow, scale, pos=torch.float64):
    """float64 roi_align, aligned, ONE sample per bin (bins <= 1 coarse pixel), the frame index clamped: [k, C, oh, ow].  ``pos``: the type the
    sample positions are formed in, in the kernels' order of operations (float32: the positions an fp32 implementation interpolates at)"""
    B, C, H, W = feat64.shape
    out = []
    for b in boxes5.to(pos):
        f = min(max(int(b[0]), 0), B - 1)
        rsw, rsh, rew, reh = (b[1:] * scale - 0.5).unbind()
        bin_h, bin_w = (reh - rsh) / oh, (rew - rsw) / ow
        assert float(bin_h) <= 1.0 and float(bin_w) <= 1.0   # (torchvision's adaptive grid is ceil(bin) samples)
        ys = (rsh + torch.arange(oh, dtype=pos) * bin_h + 0.5 * bin_h).double()
        xs = (rsw + torch.arange(ow, dtype=pos) * bin_w + 0.5 * bin_w).double()
        yl, yh, ly, yin = roi_axis64(ys, H)
        xl, xh, lx, xin = roi_axis64(xs, W)
        g = feat64[f]
        ly, lx = ly.view(1, -1, 1), lx.view(1, 1, -1)
        v = ((1 - ly) * (1 - lx) * g[:, yl][:, :, xl] + (1 - ly) * lx * g[:, yl][:, :, xh] + ly * (1 - lx) * g[:, yh][:, :, xl] + ly * lx * g[:, yh][:, :, xh])
        out.append(v * (yin.view(1, -1, 1) & xin.view(1, 1, -1)))
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def tap_inputs(case):
    H, W = TAP_MAP
    sd = 7000 + case.cout + 10 * case.cin + case.tile[0] * case.tile[1]
    return rnd(sd, case.frames, case.cin, H, W), rnd(sd + 1, case.cout, case.cin, 3, 3) / math.sqrt(9 * case.cin), tap_boxes(case)


def tap_g(case):
    """the frame-level G [B, H, W, 9 cout] (tap-major) formed in float64 and handed over as fp32: only the knot and gather kernels are under test"""
    feat_, wt, _ = tap_inputs(case)
    H, W = TAP_MAP
    return torch.einsum("oikl,bihw->bhwklo", wt.double(), feat_.double()).reshape(case.frames, H, W, 9 * case.cout).float()


def tap_ref(case, boxes=None):
    feat_, wt, b = tap_inputs(case)
    roi = roi_align64(feat_.double(), b if boxes is None else boxes, *case.tile, TAP_SCALE)
    return F.conv2d(roi, wt.double(), padding=1)


def run_taps(P, case):
    """-> (gather result NCHW on the CPU, (G, V, out) whole buffers when the case runs on slices)"""
    H, W = TAP_MAP
    (oh, ow), c = case.tile, case.cout
    boxes = tap_boxes(case)
    bd = (boxes if case.frames > 1 else boxes[:, 1:]).contiguous().to(DEV)
    G = tap_g(case)
    if not case.slices:
        taps = P.CoarseTaps(P.Feat(G.to(DEV)), c, case.kb)
        return taps.gather(bd, TAP_SCALE, oh, ow).buf.cpu().permute(0, 3, 1, 2), None
    # ldg > 9 c, ldv > c, ldo > c: G a slice of a NaN buffer; V written by the entry point itself into a slice (ops.CoarseTaps allocates it dense)
    gbuf = torch.full((case.frames, H, W, 9 * c + 8), NAN)
    gbuf[..., 4:4 + 9 * c] = G
    gf = P.Feat(gbuf.to(DEV)).slice(4, 9 * c)
    taps = P.CoarseTaps(gf, c, case.kb)
    vbuf = torch.full((case.frames, 3 * H, 3 * W, c + 12), SENTINEL, device=DEV)
    vf = P.Feat(vbuf).slice(8, c)
    L = P.L.load()
    stream = torch.cuda.current_stream().cuda_stream
    if case.frames > 1:
        P.L.check(L.prv2_coarse_tap_knots_frames(gf.ptr, case.frames, H, W, c, gf.ld, case.kb[0], case.kb[1], vf.ptr, vf.ld, stream), "coarse_tap_knots_frames")
    else:
        P.L.check(L.prv2_coarse_tap_knots(gf.ptr, H, W, c, gf.ld, case.kb[0], case.kb[1], vf.ptr, vf.ld, stream), "coarse_tap_knots")
    dense = taps.v.buf.cpu()
    taps.v = vf
    obuf = torch.full((len(boxes), oh, ow, c + 8), SENTINEL, device=DEV)
    got = taps.gather(bd, TAP_SCALE, oh, ow, out=P.Feat(obuf).slice(4, c))
    v, o = vbuf.cpu(), obuf.cpu()
    assert torch.equal(v[..., 8:8 + c], dense), "the knot table written into a slice differs from the dense one"
    assert bool((v[..., :8] == SENTINEL).all()) and bool((v[..., 8 + c:] == SENTINEL).all())
    assert bool((o[..., :4] == SENTINEL).all()) and bool((o[..., 4 + c:] == SENTINEL).all())
    return got.buf.cpu()[..., 4:4 + c].permute(0, 3, 1, 2), (gbuf, v, o)


@pytest.mark.parametrize("case", TAP_CASES + TAP_SLICE_CASES, ids=tap_id)
def test_tap_tables(P, case):
    """CoarseTaps at the production widths, on B-frame tables and on slices == float64 conv3x3(roi_align(F, boxes), W_coarse, zero padding)"""
    got, _ = run_taps(P, case)
    close(got, tap_ref(case), TAP_TOL, f"taps {tap_id(case)}")


# ---- B. the gather inside the gate kernels -----------------------------------------------------------------------------------------------
F_ = 256
FOLD_MAP, FOLD_KB = (6, 8), (0.25, 0.25)
FOLD_SHAPES = [(5, 17), (3, 16)]   # one partial tile row + a second tile column with one live column; h below the tile height, exact width
UNIT_SHAPE = (9, 17)


def fold_boxes(h, w):
    """3 tiles (x1, y1, x2, y2): two opposite frame corners and one fractional phase"""
    (H, W), (kbh, kbw) = FOLD_MAP, FOLD_KB
    bh, bw = kbh * h / TAP_SCALE, kbw * w / TAP_SCALE
    fh, fw = H / TAP_SCALE, W / TAP_SCALE
    org = [(0.0, 0.0), (fw - bw, fh - bh), (0.37 * (fw - bw), 0.61 * (fh - bh))]
    return torch.tensor([[x, y, x + bw, y + bh] for x, y in org], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def unit_inputs(h, w):
    k, (H, W) = 3, FOLD_MAP
    sd = 9000 + 100 * h + w
    return dict(x=rnd(sd, k, F_, h, w), coarse=rnd(sd + 1, 1, F_, H, W), wf=rnd(sd + 2, F_, 2 * F_, 3, 3) / math.sqrt(9 * 2 * F_), bf=rnd(sd + 3, F_) * 0.5,
                lnw=1 + 0.2 * rnd(sd + 4, F_), lnb=0.1 * rnd(sd + 5, F_), w3=rnd(sd + 6, F_, F_) / math.sqrt(F_), b3=rnd(sd + 7, F_) * 0.5,
                res=rnd(sd + 8, k, F_, h, w), boxes=fold_boxes(h, w))


@functools.lru_cache(maxsize=None)
def unit_ref(h, w):
    """roi_align -> cat -> conv(2F -> F) -> LN -> ReLU -> 1x1 -> gate (+ res) in float64; ``out`` (x, and the gate's mul) counts as hi + lo"""
    d = unit_inputs(h, w)
    b5 = torch.cat([torch.zeros(len(d["boxes"]), 1), d["boxes"]], 1)
    roi = roi_align64(d["coarse"].double(), b5, h, w, TAP_SCALE)
    xe = x2_reconstruct(d["x"]).double()
    y = F.conv2d(torch.cat([xe, roi], 1), d["wf"].double(), d["bf"].double(), padding=1)
    t = F.relu(ln64(y, d["lnw"].double(), d["lnb"].double(), 1e-6))
    z = torch.einsum("oc,nchw->nohw", d["w3"].double(), t) + d["b3"].double().view(1, -1, 1, 1)
    return xe * torch.sigmoid(z) + d["res"].double()


def run_unit(P, h, w, mode):
    """the unit's tail over ``out`` only (K = F) with the coarse half as tables (mode 'taps'), as a gathered addend ('pre'), or absent ('bare')"""
    d = unit_inputs(h, w)
    PR = P.L.PREC_NAMES["bf16x3"]
    x = feat(P, d["x"], x2=True)
    cw_a = P.pack_conv(d["wf"][:, :F_].contiguous().to(DEV), d["bf"].to(DEV), pad=1, prec=PR)
    cw_t = P.pack_conv(P.coarse_tap_weight(d["wf"][:, F_:]).to(DEV), None, prec=PR)
    taps = P.CoarseTaps(P.conv2d(feat(P, d["coarse"]), cw_t), F_, FOLD_KB)
    boxes = d["boxes"].to(DEV)
    kw = dict(taps=taps, boxes=boxes, spatial_scale=TAP_SCALE) if mode == "taps" else (dict(pre=taps.gather(boxes, TAP_SCALE, h, w)) if mode == "pre" else {})
    y = P.conv3x3_ln_gate(x, cw_a, (d["lnw"].to(DEV), d["lnb"].to(DEV)), P.pack_gate(d["w3"].to(DEV)), d["b3"].to(DEV), act=P.ACT_RELU, mul=x,
                          res=feat(P, d["res"]), pre_cin=F_, **kw)
    assert last_kernel(P) == KERNELS["gx2"].format("bf16x3"), last_kernel(P)
    return y.buf.cpu()


@pytest.mark.parametrize("hw", FOLD_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_folded_gather_is_the_gathered_addend_bit_for_bit(P, hw):
    folded, pre, bare = (run_unit(P, *hw, m) for m in ("taps", "pre", "bare"))
    assert bool(torch.isfinite(pre).all()) and not torch.equal(pre, bare)
    assert torch.equal(folded, pre), (int((folded != pre).sum()), float((folded - pre).abs().max()))


def test_gated_unit_on_the_taps_path_vs_float64(P):
    h, w = UNIT_SHAPE
    close(run_unit(P, h, w, "taps").permute(0, 3, 1, 2), unit_ref(h, w), UNIT_TOL, f"unit {h}x{w} taps")
