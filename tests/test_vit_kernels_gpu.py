"""GPU parity of the transformer path -- csrc/attention.hip (attention_f32_kernel, the pre-pass attention_bf16x3_kernel, attention_qkvss_kernel,
the bias packer), csrc/gemm_ss.hip (the 64 / 128 / 256 tiles, two and four LDS stages, the blocked tile order, the persistent walker, split_ss_kernel)
and layernorm_kernel<V, true> -- against plain torch in float64 on the CPU, at the smallest shapes that still reach each launch path and on the
edges of the 64-key / 128-query tiles.  Nothing here shares arithmetic with the kernels: the split-swizzled operand format is restated from the
header text alone (``ss_encode`` / ``ss_decode``, include/prv2.h "Split-swizzled"), every split-swizzled input is built by ``ss_encode`` and every
split-swizzled output is read by ``ss_decode`` -- no kernel's output is ever decoded by another kernel.  The tables, references, tolerances and
float32 emulations need no GPU and no library: tests/test_vit_kernels_host.py checks them (the launch path of every row against a restatement
of gemm_ss_impl's predicates, the edge every attention shape is listed for, the emulations' share of every tolerance, discrimination).

Destinations are NaN where the op must write and hold a sentinel beside it.  Every comparison prints ``err / tol`` before it asserts."""
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENT = -7.5                 # what every column beside a destination slice holds before and after
LOG2E = np.float32(1.4426950408889634)
Q_SCALE = float(np.float32(0.125) * LOG2E)      # hd^-0.5 log2 e at head_dim 64, the float32 product (== ops.Q_SCALE, asserted on the GPU side)
PREC_F32, PREC_BF16X3, PREC_BF16 = 0, 1, 2      # include/prv2.h
ACT_NONE, ACT_GELU = 0, 2


@pytest.fixture(scope="module")
def P():
    from patchrefinerv2_amd import ops
    ops.L.load()
    assert (ops.L.PREC_F32, ops.L.PREC_BF16X3, ops.L.PREC_BF16, ops.ACT_NONE, ops.ACT_GELU) == (PREC_F32, PREC_BF16X3, PREC_BF16, ACT_NONE, ACT_GELU)
    assert ops.Q_SCALE == Q_SCALE
    return ops


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def cdiv(a, b):
    return (a + b - 1) // b


def roundup(a, b):
    return cdiv(a, b) * b


def within(got, ref, tol, what):
    """max(|got - ref| / tol) <= 1 (tol: a number or a tensor of ref's shape), the output finite; prints the share of the tolerance used"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - ref.double()).abs_()
    emax = float(err.max())
    ratio = float(err.div_(torch.as_tensor(tol, dtype=torch.float64)).max())
    print(f"[vit] {what}: err {emax:.3e} err/tol {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: max|d| = {emax:.3e}, {ratio:.3f} of the tolerance"
    return ratio


# ---- 0. the split-swizzled format, from the header text (include/prv2.h "Split-swizzled") ------------------------------------------------
# A row of C channels (C % 32 == 0) occupies 4 C bytes: per 32 channels one 128-byte group of eight 16-byte slots; logical slot s = 0..3 holds
# the bf16 hi of channels 8s..8s+7, s = 4..7 the bf16 lo of channels 8(s-4)..8(s-4)+7; logical slot s is stored at slot s ^ ((row >> 1) & 7),
# row = the GLOBAL row.  hi = bf16_rne(x), lo = bf16_rne(x - hi).
def bf16(x):
    return x.to(torch.bfloat16).float()


def split(x):
    hi = bf16(x)
    return hi, bf16(x - hi)


def ss_key(row):
    return (row >> 1) & 7


def _slot_index(rows, groups, row0, key):
    """[rows, groups, 8, 8] gather index along the slot axis: XOR is its own inverse, so stored slot t holds logical slot t ^ key and back"""
    k = key(torch.arange(row0, row0 + rows))
    return (torch.arange(8)[None, :] ^ k[:, None])[:, None, :, None].expand(rows, groups, 8, 8)


def ss_encode(x, row0=0, key=ss_key, swap=False):
    """float32 [rows, C] -> the float32 container [rows, C] of its split-swizzled rows (``key`` / ``swap``: the deliberately wrong variants)"""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] % 32 == 0, x.shape
    rows, c = x.shape
    hi, lo = split(x.contiguous())
    if swap:
        hi, lo = lo, hi
    logical = torch.cat([hi.view(rows, c // 32, 4, 8), lo.view(rows, c // 32, 4, 8)], 2).to(torch.bfloat16).view(torch.int16)
    stored = torch.gather(logical, 2, _slot_index(rows, c // 32, row0, key)).contiguous()
    return stored.view(rows, 2 * c).view(torch.float32)


def ss_decode(container, row0=0, key=ss_key):
    """the float32 container [rows, C] -> (hi, lo) as float32 [rows, C]"""
    assert container.dtype == torch.float32 and container.dim() == 2 and container.shape[1] % 32 == 0, container.shape
    rows, c = container.shape
    stored = container.contiguous().view(torch.int16).view(rows, c // 32, 8, 8)
    logical = torch.gather(stored, 2, _slot_index(rows, c // 32, row0, key)).contiguous().view(torch.bfloat16).float()
    return logical[:, :, :4].reshape(rows, c), logical[:, :, 4:].reshape(rows, c)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def read_ss(container, what):
    """a kernel's split-swizzled rows -> hi + lo (exact in float32: both halves are 8-bit significands at most 2^-8 apart), after the check
    that the pair is a split: finite, lo == bf16((hi + lo) - hi), and lo no larger than half a bf16 ulp of hi (2^-8 |hi|)"""
    hi, lo = ss_decode(container.detach().cpu())
    assert bool(torch.isfinite(hi).all() and torch.isfinite(lo).all()), f"{what}: non-finite split-swizzled rows"
    v = hi + lo
    assert torch.equal(lo, bf16(v - hi)), f"{what}: lo is not the bf16 of the remainder"
    assert bool((lo.abs() <= 2.0 ** -8 * hi.abs()).all()), f"{what}: lo larger than half an ulp of hi"
    return v


# ---- a. split_ss: the format itself -------------------------------------------------------------------------------------------------
SPLIT_CASES = [
    (1, 32, 32),
    (16, 32, 32),       # rows 0..15 take all eight swizzle keys
    (17, 96, 100),      # ldx > c: NaN in the pad columns
    (33, 160, 160),
]
# +-0; exact in bf16 (lo == 0); hi rounds up (lo < 0), both signs; the two ties (to even: down, lo > 0, and up, lo < 0); +-1e30; 24 significant bits
SPECIALS = [0.0, -0.0, 1.0, -2.5, 0.15625, 1 + 3 * 2.0 ** -9, -(1 + 3 * 2.0 ** -9), 1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1e30, -1e30, 3.0000001]
TINY_SHAPE = (9, 64)    # row r: magnitudes 1e-(30 + r), 1e-30 .. 1e-38 (the last below the smallest normal number)


def split_input(case):
    """-> [rows, ldx]: randn x 3, the last row's first columns the specials, NaN in the columns [c, ldx)"""
    rows, c, ldx = case
    buf = torch.full((rows, ldx), NAN)
    buf[:, :c] = rnd(10 + SPLIT_CASES.index(case), rows, c) * 3
    buf[-1, :len(SPECIALS)] = torch.tensor(SPECIALS)
    return buf


def tiny_input():
    rows, c = TINY_SHAPE
    mant = 1 + 8 * torch.rand(rows, c, generator=torch.Generator().manual_seed(20))
    sign = 1 - 2 * (torch.arange(c) % 2).float()
    return (mant.double() * sign * 10.0 ** -(30 + torch.arange(rows).double())[:, None]).float()


def tiny_tol(x):
    """2^-17 |x| + 2^-126: for 2^e <= |x| < 2^(e + 1) the remainder x - hi is at most 2^(e - 8), and below that its bf16 rounding errs by at
    most 2^(e - 17) <= 2^-17 |x| (sharp for x just above a power of two); anything under the smallest normal number may be flushed"""
    return 2.0 ** -17 * x.double().abs() + 2.0 ** -126


@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_split_ss_is_the_header_format_bit_for_bit(P, case):
    rows, c, ldx = case
    buf = split_input(case)
    got = P.split_ss(buf.to(DEV)[:, :c]).cpu()
    want = ss_encode(buf[:, :c])
    diff = int((got.view(torch.int32) != want.view(torch.int32)).sum())
    print(f"[vit] a split_ss {rows}x{c} ld {ldx}: {diff} of {rows * c} words differ")
    assert same_bits(got, want)


def test_split_ss_tiny_magnitudes_value_bound(P):
    x = tiny_input()
    hi, lo = ss_decode(P.split_ss(x.to(DEV)).cpu())
    within(hi.double() + lo.double(), x.double(), tiny_tol(x), "a split_ss 1e-30..1e-38")


# ---- b. layernorm_ss ---------------------------------------------------------------------------------------------------------------------
# (rows, c, ldx): both sides of every V boundary of layernorm_kernel<V, true> (c <= 256, 512, 1024, else 8), 4 rows per block
LN_CASES = [
    (1, 32, 32),
    (5, 256, 256),      # a ragged second block
    (6, 288, 292),      # ldx > c
    (3, 512, 512),
    (3, 544, 544),
    (2, 1024, 1024),
    (2, 1056, 1056),
    (2, 2048, 2052),
]
LN_REFUSED = (48, 2080)     # c % 32 != 0; c > 2048
LN_EPS = 1e-6


def ln_inputs(case):
    """-> (x [rows, ldx] with NaN in the pad columns, weight, bias)"""
    rows, c, ldx = case
    i = LN_CASES.index(case)
    buf = torch.full((rows, ldx), NAN)
    buf[:, :c] = rnd(30 + i, rows, c) * 3 + 1
    return buf, 1 + 0.5 * rnd(40 + i, c), rnd(50 + i, c)


def layernorm_any(x, w, b, dtype):
    return F.layer_norm(x.to(dtype), x.shape[-1:], w.to(dtype), b.to(dtype), LN_EPS)


@functools.lru_cache(maxsize=None)
def ln_ref(case):
    buf, w, b = ln_inputs(case)
    return layernorm_any(buf[:, :case[1]], w, b, torch.float64)


def ln_tol(ref):
    """1e-5 max(1, max|ref|) -- test_layernorm's bar -- + 2^-17 |ref| for the 16 significand bits of the pair"""
    return 1e-5 * max(1.0, float(ref.abs().max())) + 2.0 ** -17 * ref.abs()


def ln_emulation(case):
    buf, w, b = ln_inputs(case)
    hi, lo = split(layernorm_any(buf[:, :case[1]], w, b, torch.float32))
    return hi + lo


@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_layernorm_ss(P, case):
    rows, c, ldx = case
    buf, w, b = ln_inputs(case)
    xd, wd, bd = buf.to(DEV), w.to(DEV), b.to(DEV)
    y_ss = torch.full((rows, c), NAN, device=DEV)
    P.layernorm_ss(xd, rows, c, ldx, wd, bd, LN_EPS, y_ss)
    ref = ln_ref(case)
    within(read_ss(y_ss, "layernorm_ss"), ref, ln_tol(ref), f"b layernorm_ss {rows}x{c} ld {ldx}")
    y = torch.full((rows, c), NAN, device=DEV)
    P.layernorm_rows(xd, rows, c, ldx, wd, bd, LN_EPS, P.ACT_NONE, y, c)
    assert same_bits(y_ss.cpu(), ss_encode(y.cpu())), "layernorm_ss != the split of layernorm's rows"


@pytest.mark.parametrize("c", LN_REFUSED)
def test_layernorm_ss_refuses(P, c):
    x, w = torch.zeros(2, c, device=DEV), torch.ones(c, device=DEV)
    with pytest.raises(RuntimeError):
        P.layernorm_ss(x, 2, c, c, w, w, LN_EPS, torch.empty_like(x))


# ---- c. gemm_ss / gemm_ss_qkv -----------------------------------------------------------------------------------------------------------
TILE_ENV, PERSIST_ENV, PPB_ENV = "PRV2_GEMM_SS_TILE", "PRV2_GSS_PERSIST", "PRV2_GSS_PPB"
GEMM_SWITCHES = (TILE_ENV, PERSIST_ENV, PPB_ENV, "PRV2_GEMM_SS_BLOCKED", "PRV2_GEMM_SS_SMALL", "PRV2_GEMM_SS_DEEP", "PRV2_GSS_DEFER")
SMALL_EPIS = ("E0", "E1", "E2", "E3", "E4", "E5", "E6")
LARGE_EPIS = ("E4", "E6")
T128 = ({TILE_ENV: "128"},)
T256 = ({TILE_ENV: "256", PERSIST_ENV: "1"}, {TILE_ENV: "256", PERSIST_ENV: "0"})
WALK = ({TILE_ENV: "256", PERSIST_ENV: "1", PPB_ENV: "1"}, {TILE_ENV: "256", PERSIST_ENV: "1", PPB_ENV: "2"})


def _gemm(route, M, K, N, tile, envs=({},), epis=SMALL_EPIS, heads=0):
    epis = tuple(e for e in epis if N % 32 == 0 or e not in ("E5", "E6")) + (("E7",) if heads else ())
    return NS(route=route, M=M, K=K, N=N, tile=tile, envs=envs, epis=epis, heads=heads)


# route: tile and LDS stages / tile order / walk; the host file checks every row against gemm_ss_impl's predicates
GEMM_CASES = [
    _gemm("64x4", 1, 32, 8, 64),                            # one slab: fewer than the stages
    _gemm("64x4", 65, 96, 72, 64),
    _gemm("64x4", 64, 160, 64, 64),                         # 5 slabs: the ring of 4 stages wraps
    _gemm("64x4", 130, 128, 96, 64),
    _gemm("64x4", 65, 96, 192, 64, heads=1),
    _gemm("64x4", 257, 64, 384, 64, heads=2),
    _gemm("64x2", 1025, 96, 1000, 64),                      # 272 tiles of 64: two stages
    _gemm("128", 128, 32, 128, 128, T128),
    _gemm("128", 129, 64, 136, 128, T128),
    _gemm("128-blocked", 8200, 32, 1024, 128, T128, LARGE_EPIS),    # 65 row tiles walk as 68: 3 rows of ids idle
    _gemm("256", 256, 64, 256, 256, T256),
    _gemm("256", 257, 96, 264, 256, T256),
    _gemm("256-blocked", 2050, 32, 2048, 256, T256, LARGE_EPIS),
    _gemm("256-walk", 4400, 96, 4096, 256, WALK, LARGE_EPIS),       # 18 x 16 tiles -> 320 ids on 256 workgroups, 3 slabs: the parity carries
]
EPI = {
    "E0": NS(bias=False, gelu=False, gamma=False, ss=False),
    "E1": NS(bias=True, gelu=False, gamma=False, ss=False),
    "E2": NS(bias=True, gelu=True, gamma=False, ss=False),      # bias + GELU into fp32 rows
    "E3": NS(bias=True, gelu=False, gamma=True, ss=False),      # bias + gamma + residual, out of place
    "E4": NS(bias=True, gelu=False, gamma=True, ss=False),      # the same in place in the columns [4, 4 + N) of N + 8: ldy = ld_res > N
    "E5": NS(bias=True, gelu=False, gamma=False, ss=True),
    "E6": NS(bias=True, gelu=True, gamma=False, ss=True),
    "E7": NS(bias=True, gelu=False, gamma=False, ss=True),      # gemm_ss_qkv: the q third times Q_SCALE behind the bias
}
GEMM_RUNS = [(ci, ei, epi) for ci, c in enumerate(GEMM_CASES) for ei in range(len(c.envs)) for epi in c.epis]


def gemm_run_id(run):
    ci, ei, epi = run
    c = GEMM_CASES[ci]
    return f"{c.route}-{c.M}x{c.K}x{c.N}-env{ei}-{epi}"


def gelu64(x):
    return 0.5 * x * (1 + torch.special.erf(x * 0.7071067811865476))


def gelu_fast32(v):
    """gelu_fast of csrc/common.h in numpy float32, operation for operation (v_rcp_f32 as 1 / x, v_exp_f32 as exp2)"""
    f = np.float32
    v = np.asarray(v, dtype=f)
    x = v * f(0.70710678118654752440)
    ax = np.abs(x)
    t = f(1.0) / (f(1.0) + f(0.3275911) * ax)
    p = f(1.061405429) * t
    p = (p - f(1.453152027)) * t
    p = (p + f(1.421413741)) * t
    p = (p - f(0.284496736)) * t
    p = (p + f(0.254829592)) * t
    r = f(1.0) - p * np.exp2(ax * ax * f(-1.44269504088896340736))
    return f(0.5) * v * (f(1.0) + np.copysign(r, x))


@functools.lru_cache(maxsize=None)
def gelu_term():
    """-> (d, g): d = max|gelu_fast32 - float64 GELU| over a dense grid of [-8, 8] (the source comment claims 4.7e-7), g = 2 d, the GELU term of
    the GEMM tolerance"""
    v = np.linspace(-8.0, 8.0, 2 ** 21 + 1).astype(np.float32)
    d = float(np.abs(gelu_fast32(v).astype(np.float64) - gelu64(torch.from_numpy(v).double()).numpy()).max())
    return d, 2 * d


@functools.lru_cache(maxsize=None)
def gemm_inputs(ci):
    """a: what the kernel is given (ss_encode of randn) and what that container holds (hi + lo); w randn / sqrt(K); bias, gamma, res.
    The bias is 0.1 randn as in tests/test_hip_ops.py: the tolerance has no term of its own for the rounding of a split-swizzled OUTPUT
    (2^-17 of the value); its 3 2^-18 mag term pays for it as long as the bias does not lift |value| far above mag.  gamma is 1 + 0.1 randn, a
    LayerScale away from zero: at gamma = 0 the tolerance shrinks to 2^-23 |res|, half of which is the final rounding alone"""
    c = GEMM_CASES[ci]
    a_ss = ss_encode(rnd(100 + ci, c.M, c.K))
    hi, lo = ss_decode(a_ss)
    return NS(a_ss=a_ss, a=hi + lo, w=rnd(120 + ci, c.N, c.K) / c.K ** 0.5, bias=0.1 * rnd(140 + ci, c.N), gamma=1 + 0.1 * rnd(160 + ci, c.N),
              res=rnd(180 + ci, c.M, c.N))


@functools.lru_cache(maxsize=2)
def gemm_core(ci):
    """float64: -> (A W^T, |A| |W|^T)"""
    inp = gemm_inputs(ci)
    a, w = inp.a.double(), inp.w.double()
    return a @ w.t(), a.abs() @ w.abs().t()


def q_scale_columns(c):
    s = torch.ones(c.N, dtype=torch.float64)
    s[:c.heads * 64] = Q_SCALE
    return s


def gemm_ref(ci, epi):
    """-> (float64 reference, per-element tolerance).
    tol = 2 [(3 2^-18 + (K + 2) 2^-24) mag + 2^-23 |pre-activation|] |gamma| + 2^-23 |res| + g, mag = |A| |W|^T from the operand the kernel
    reads: the dropped lo lo product is 2^-18 mag, each of the two bf16 roundings of the weights' and the operand's lo another 2^-18 mag, fp32
    accumulation of 3 K / 32 MFMA results of 32 products (K + 2) 2^-24 mag; 2^-23 for the roundings of bias, gamma and residual; g = gelu_term()
    (GELU is 1.13-Lipschitz, which the factor 2 pays for).  E7: the q columns, and their tolerance, times Q_SCALE"""
    c, inp, e = GEMM_CASES[ci], gemm_inputs(ci), EPI[epi]
    acc, mag = gemm_core(ci)
    pre = acc + inp.bias.double() if e.bias else acc
    tol = (mag * (3 * 2.0 ** -18 + (c.K + 2) * 2.0 ** -24)).add_(pre.abs(), alpha=2.0 ** -23).mul_(2)
    ref = gelu64(pre) if e.gelu else pre
    if e.gamma:
        ref = ref * inp.gamma.double() + inp.res.double()
        tol = tol.mul_(inp.gamma.double().abs()).add_(inp.res.double().abs(), alpha=2.0 ** -23)
    if e.gelu:
        tol = tol.add_(gelu_term()[1])
    if epi == "E7":
        ref, tol = ref * q_scale_columns(c), tol.mul_(q_scale_columns(c))
    return ref, tol


def three_products(ah, al, w):
    """float32: the kernels' lo hi + hi lo + hi hi (smallest first) of a pre-split operand with the split of w"""
    wh, wl = split(w)
    return (al @ wh.t() + ah @ wl.t()) + ah @ wh.t()


def gemm_emulation(ci, epi, drop_lo_hi=False, gelu_first=False, scale_first=False, a_key=ss_key, a_swap=False):
    """the case in float32 on the CPU, hi / lo arithmetic included; the keywords are the deliberately wrong variants: the lo hi product dropped,
    GELU in front of the bias, the q scale in front of the bias, the operand read with another swizzle key or with hi and lo slots exchanged"""
    c, inp, e = GEMM_CASES[ci], gemm_inputs(ci), EPI[epi]
    ah, al = ss_decode(inp.a_ss, key=a_key)
    if a_swap:
        ah, al = al, ah
    t = three_products(ah, al * (0.0 if drop_lo_hi else 1.0), inp.w)
    s = q_scale_columns(c).float() if epi == "E7" else None
    if scale_first:
        t = t * s
    if e.gelu and gelu_first:
        t = torch.from_numpy(gelu_fast32(t.numpy()))
    if e.bias:
        t = t + inp.bias
    if e.gelu and not gelu_first:
        t = torch.from_numpy(gelu_fast32(t.numpy()))
    if e.gamma:
        t = t * inp.gamma + inp.res
    if s is not None and not scale_first:
        t = t * s
    if e.ss:
        hi, lo = split(t)
        t = hi + lo
    return t


def run_gemm(P, ci, epi):
    """-> the kernel's result on the CPU, decoded where it is split-swizzled"""
    c, inp, e = GEMM_CASES[ci], gemm_inputs(ci), EPI[epi]
    a = inp.a_ss.to(DEV)
    cw = P.pack_conv(inp.w.to(DEV), inp.bias.to(DEV) if e.bias else None, prec=PREC_BF16X3)
    act = ACT_GELU if e.gelu else ACT_NONE
    if epi == "E7":
        return read_ss(P.gemm_ss_qkv(a, cw, c.heads), "gemm_ss_qkv")
    if e.ss:
        out = torch.full((c.M, c.N), NAN, device=DEV)
        P.gemm_ss(a, cw, out=out, out_ss=True, act=act)
        return read_ss(out, "gemm_ss")
    if epi == "E4":
        wide = torch.full((c.M, c.N + 8), SENT)
        wide[:, 4:4 + c.N] = inp.res
        wide = wide.to(DEV)
        x = wide[:, 4:4 + c.N]
        P.gemm_ss(a, cw, out=x, gamma=inp.gamma.to(DEV), res=x)
        got = wide.cpu()
        assert bool((got[:, :4] == SENT).all() and (got[:, 4 + c.N:] == SENT).all()), "columns beside the destination slice were written"
        return got[:, 4:4 + c.N]
    out = torch.full((c.M, c.N), NAN, device=DEV)
    if e.gamma:
        P.gemm_ss(a, cw, out=out, gamma=inp.gamma.to(DEV), res=inp.res.to(DEV))
    else:
        P.gemm_ss(a, cw, out=out, act=act)
    return out.cpu()


@pytest.mark.parametrize("run", GEMM_RUNS, ids=gemm_run_id)
def test_gemm_ss(P, run, monkeypatch):
    ci, ei, epi = run
    c = GEMM_CASES[ci]
    for name in GEMM_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in c.envs[ei].items():
        monkeypatch.setenv(name, value)
    got = run_gemm(P, ci, epi)
    kernel = P.L.load().prv2_last_kernel().decode()
    assert kernel == f"gemm_ss_kernel<{c.tile},bf16x3>", kernel
    ref, tol = gemm_ref(ci, epi)
    within(got, ref, tol, f"c gemm_ss {gemm_run_id(run)}")


# ---- d. attention ------------------------------------------------------------------------------------------------------------------------
AT_BQ, AT_BK = 128, 64      # queries per workgroup (4 waves x 32), keys per tile
# (b, ntok, heads)
ATT_SHAPES = [
    (1, 1, 1),
    (2, 33, 1),         # an odd ntok: the second image starts at an odd global row
    (1, 63, 2),         # only a masked tile
    (1, 64, 1),         # no masked tile
    (3, 65, 2),         # one key in the masked tile
    (1, 127, 1),
    (1, 128, 1),
    (2, 129, 3),        # one key in the masked tile, one query in the second query block: three of its four waves retire early
    (1, 193, 1),
    (1, 257, 2),        # the same with two heads: the 1-D grid decode
]
ATT_LD_EXTRA = {(2, 129, 3): 4}     # bias rows of roundup(ntok, 64) + 4 columns
ATT_DENSE_IMAGE = (3, 65, 2)        # its packed image comes from rows with ld_bias == ntok, which the packer accepts and the kernels do not
ATT_BF16_ONCE = (3, 65, 2)          # prec = bf16 runs the same kernel
SPIKE_FACTORS = (4.0, 5.0, 6.0)
F32_BAR, BF16_BAR = 1e-5, 4e-5      # test_attention's bars, times max(1, max|ref|)


def att_id(s):
    return f"{s[0]}x{s[1]}x{s[2]}h"


def spike_keys(ntok):
    """keys 2, ntok - 1 and the first key of the last tile where that is another key"""
    if ntok < 3:
        return []
    keys = [2, ntok - 1]
    first = (ntok - 1) // AT_BK * AT_BK
    return keys + ([first] if first not in keys else [])


def spike_query(i, ntok):
    return (5 + 11 * i) % ntok


@functools.lru_cache(maxsize=None)
def att_inputs(shape):
    """q, k, v [b, heads, ntok, 64] randn with spike keys (4 - 6 x a query row: the row maximum moves from tile to tile, into the masked one);
    bias [heads, ntok, ntok] = randn 2 - 12 (softmax is shift invariant; a phantom key of score 0 would take nearly all the mass) and its rows
    [heads, ntok, ld] with NaN in every pad column; the fp32 qkv rows [3][heads][64] and the container of [q Q_SCALE | k | v]"""
    b, n, h = shape
    i = ATT_SHAPES.index(shape)
    q, k, v = rnd(200 + i, b, h, n, 64), rnd(220 + i, b, h, n, 64), rnd(240 + i, b, h, n, 64)
    for j, key in enumerate(spike_keys(n)):
        k[:, :, key] = SPIKE_FACTORS[j] * q[:, :, spike_query(j, n)]
    bias = rnd(260 + i, h, n, n) * 2 - 12
    ld = roundup(n, AT_BK) + ATT_LD_EXTRA.get(shape, 0)
    rows = torch.full((h, n, ld), NAN)
    rows[:, :, :n] = bias
    flat = [t.permute(0, 2, 1, 3).reshape(b * n, h * 64) for t in (q, k, v)]
    qkv_ss = ss_encode(torch.cat([flat[0] * torch.tensor(Q_SCALE, dtype=torch.float32), flat[1], flat[2]], 1))
    return NS(q=q, k=k, v=v, bias=bias, bias_rows=rows, qkv=torch.cat(flat, 1).contiguous(), qkv_ss=qkv_ss)


def as_rows(o):
    b, h, n, d = o.shape
    return o.permute(0, 2, 1, 3).reshape(b * n, h * d)


def attention64(q, k, v, bias=None):
    s = q.double() @ k.double().transpose(-1, -2) / 8
    if bias is not None:
        s = s + bias.double()
    return as_rows(s.softmax(-1) @ v.double())


@functools.lru_cache(maxsize=None)
def att_ref(shape, with_bias):
    inp = att_inputs(shape)
    return attention64(inp.q, inp.k, inp.v, inp.bias if with_bias else None)


def att_tol(ref, bar):
    return bar * max(1.0, float(ref.abs().max()))


def attention_split32(q, k, v, bias=None, out_ss=False, drop_lo_hi=False, bias_scale=LOG2E):
    """the bf16x3 kernels in float32 on the CPU: base-2 scores of the split operands (lo hi + hi lo + hi hi), + bias log2 e, an exact softmax,
    P V with both operands split; -> rows.  ``drop_lo_hi`` / ``bias_scale``: the deliberately wrong variants"""
    qh, ql = split(q * torch.tensor(Q_SCALE, dtype=torch.float32))
    kh, kl = split(k)
    vh, vl = split(v)
    kt_h, kt_l = kh.transpose(-1, -2), kl.transpose(-1, -2)
    s = ((0.0 if drop_lo_hi else 1.0) * (ql @ kt_h) + qh @ kt_l) + qh @ kt_h
    if bias is not None:
        s = s + bias * torch.tensor(float(bias_scale), dtype=torch.float32)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    ph, pl = split(p)
    o = as_rows(((pl @ vh + ph @ vl) + ph @ vh) / p.sum(-1, keepdim=True))
    if out_ss:
        hi, lo = split(o)
        o = hi + lo
    return o


def att_bias_arg(P, shape, kind):
    inp = att_inputs(shape)
    if kind == "none":
        return None
    if kind == "rows":
        return inp.bias_rows.to(DEV)
    src = inp.bias.contiguous() if shape == ATT_DENSE_IMAGE else inp.bias_rows
    return P.pack_attention_bias(src.to(DEV), shape[1])


def read_att(out, shape, out_ss, what):
    """fp32 rows as they are; split-swizzled rows image by image with the image's first GLOBAL row"""
    b, n, _ = shape
    if not out_ss:
        return out.cpu()
    whole = read_ss(out, what)
    hi, lo = zip(*(ss_decode(out[i * n:(i + 1) * n].cpu(), row0=i * n) for i in range(b)))
    assert torch.equal(torch.cat(hi) + torch.cat(lo), whole), "row0 does not shift the key"
    return whole


@pytest.mark.parametrize("shape", ATT_SHAPES, ids=att_id)
def test_attention_f32(P, shape):
    b, n, h = shape
    qkv = att_inputs(shape).qkv.to(DEV)
    for kind in ("none", "rows"):
        got = P.attention(qkv, b, n, h, PREC_F32, bias=att_bias_arg(P, shape, kind))
        ref = att_ref(shape, kind != "none")
        within(got, ref, att_tol(ref, F32_BAR), f"d attention f32 {att_id(shape)} bias {kind}")


def run_prepass(P, shape, kind, out_ss, prec=PREC_BF16X3):
    b, n, h = shape
    return P.attention(att_inputs(shape).qkv.to(DEV), b, n, h, prec, bias=att_bias_arg(P, shape, kind), out_ss=out_ss)


@pytest.mark.parametrize("shape", ATT_SHAPES, ids=att_id)
def test_attention_pre_pass(P, shape):
    for kind in ("none", "rows", "image"):
        ref = att_ref(shape, kind != "none")
        for out_ss in (False, True):
            what = f"d attention pre-pass {att_id(shape)} bias {kind} {'ss' if out_ss else 'fp32'} rows"
            within(read_att(run_prepass(P, shape, kind, out_ss), shape, out_ss, what), ref, att_tol(ref, BF16_BAR), what)
    if shape == ATT_BF16_ONCE:
        ref = att_ref(shape, True)
        within(run_prepass(P, shape, "rows", False, PREC_BF16).cpu(), ref, att_tol(ref, BF16_BAR), f"d attention prec bf16 {att_id(shape)}")


@pytest.mark.parametrize("shape", ATT_SHAPES, ids=att_id)
def test_attention_qkv_ss(P, shape):
    """attention_qkvss_kernel alone: its operand is ss_encode of [q Q_SCALE | k | v], not a GEMM's output; and bit-equal to the pre-pass kernel"""
    b, n, h = shape
    qkv_ss = att_inputs(shape).qkv_ss.to(DEV)
    for kind in ("none", "rows", "image"):
        ref = att_ref(shape, kind != "none")
        for out_ss in (False, True):
            what = f"d attention qkv-ss {att_id(shape)} bias {kind} {'ss' if out_ss else 'fp32'} rows"
            got = P.attention_qkv_ss(qkv_ss, b, n, h, bias=att_bias_arg(P, shape, kind), out_ss=out_ss)
            within(read_att(got, shape, out_ss, what), ref, att_tol(ref, BF16_BAR), what)
            assert same_bits(got.cpu(), run_prepass(P, shape, kind, out_ss).cpu()), f"{what}: not the pre-pass kernel's bits"


# ---- e. pack_attention_bias ---------------------------------------------------------------------------------------------------------------
PACK_CASES = [(1, 1, 64), (2, 65, 65), (3, 129, 192)]       # (heads, ntok, ld_bias)


def bias_image(rows, ntok):
    """the layout stated in csrc/attention.hip: [head][block of 32 queries][tile of 64 keys][i = 4 t + g][lane][4], q = 32 block + (lane & 31),
    key = 64 tile + 32 t + 8 g + 4 (lane >> 5) + e; the float32 product bias * log2 e, zero for q >= ntok or key >= ntok.  rows: numpy
    float32 [heads, ntok, ld]"""
    heads = rows.shape[0]
    q32n, ktn = cdiv(ntok, AT_BQ) * (AT_BQ // 32), cdiv(ntok, AT_BK)
    blk, tile, i, lane, e = np.meshgrid(np.arange(q32n), np.arange(ktn), np.arange(8), np.arange(64), np.arange(4), indexing="ij")
    q = 32 * blk + (lane & 31)
    key = 64 * tile + 32 * (i >> 2) + 8 * (i & 3) + 4 * (lane >> 5) + e
    live = (q < ntok) & (key < ntok)
    img = np.zeros((heads,) + q.shape, dtype=np.float32)
    for hd in range(heads):
        img[hd][live] = rows[hd][q[live], key[live]] * LOG2E
    return img.reshape(-1)


def image_bytes(heads, ntok):
    return heads * cdiv(ntok, AT_BQ) * (AT_BQ // 32) * cdiv(ntok, AT_BK) * 8 * 64 * 16


def pack_input(case):
    heads, n, ld = case
    rows = torch.full((heads, n, ld), NAN)
    rows[:, :, :n] = rnd(300 + PACK_CASES.index(case), heads, n, n) * 2 - 12
    return rows


@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: f"{c[0]}h-{c[1]}-ld{c[2]}")
def test_pack_attention_bias(P, case):
    heads, n, ld = case
    rows = pack_input(case)
    img = P.pack_attention_bias(rows.to(DEV), n)
    assert (img.heads, img.ntok) == (heads, n)
    assert P.L.load().prv2_attention_bias_image_bytes(heads, n) == image_bytes(heads, n) == img.image.numel() * 4
    got, want = img.image.cpu().numpy(), bias_image(rows.numpy(), n)
    assert np.isfinite(got).all() and np.array_equal(got.view(np.int32), want.view(np.int32))


# ---- f. one ViT block on the production call chain --------------------------------------------------------------------------------------------
BLOCK = NS(B=2, N=65, D=128, heads=2, hidden=512)


@functools.lru_cache(maxsize=None)
def block_inputs():
    d, hid = BLOCK.D, BLOCK.hidden
    lin = lambda s, n, k: (rnd(s, n, k) / k ** 0.5, 0.1 * rnd(s + 1, n))  # noqa: E731
    return NS(x=rnd(400, BLOCK.B * BLOCK.N, d), n1=(1 + 0.1 * rnd(401, d), 0.1 * rnd(402, d)), n2=(1 + 0.1 * rnd(403, d), 0.1 * rnd(404, d)),
              qkv=lin(410, 3 * d, d), proj=lin(412, d, d), fc1=lin(414, hid, d), fc2=lin(416, d, hid), ls1=1 + 0.1 * rnd(420, d), ls2=1 + 0.1 * rnd(421, d))


def heads_of(rows, third):
    """columns [third][heads][64] of qkv rows -> [B, heads, N, 64]"""
    d = BLOCK.D
    return rows[:, third * d:(third + 1) * d].reshape(BLOCK.B, BLOCK.N, BLOCK.heads, 64).permute(0, 2, 1, 3)


@functools.lru_cache(maxsize=None)
def block64(q_bias_gain=1.0):
    """the DINOv2 block (attention.py, mlp.py, layer_scale.py) in float64.  ``q_bias_gain`` 1 / Q_SCALE is the deliberately wrong variant: the
    q scale of the qkv Linear in front of its bias"""
    p = block_inputs()
    dd = lambda t: t.double()  # noqa: E731
    x = dd(p.x)
    gain = torch.ones(3 * BLOCK.D, dtype=torch.float64)
    gain[:BLOCK.D] = q_bias_gain
    qkv = layernorm_any(x, *p.n1, torch.float64) @ dd(p.qkv[0]).t() + dd(p.qkv[1]) * gain
    a = attention64(heads_of(qkv, 0), heads_of(qkv, 1), heads_of(qkv, 2))
    x = (a @ dd(p.proj[0]).t() + dd(p.proj[1])) * dd(p.ls1) + x
    f = gelu64(layernorm_any(x, *p.n2, torch.float64) @ dd(p.fc1[0]).t() + dd(p.fc1[1]))
    return (f @ dd(p.fc2[0]).t() + dd(p.fc2[1])) * dd(p.ls2) + x


@functools.lru_cache(maxsize=None)
def block_emulation():
    """the same block in float32 on the CPU the way the chain computes it: every Linear operand as bf16 hi + lo with the three products, the q third
    times Q_SCALE behind the bias, base-2 softmax (exact, one pass), gelu_fast; float32 accumulation"""
    p = block_inputs()
    lin = lambda t, wb: three_products(*split(t), wb[0]) + wb[1]  # noqa: E731
    qkv = lin(layernorm_any(p.x, *p.n1, torch.float32), p.qkv)
    a = attention_split32(heads_of(qkv, 0), heads_of(qkv, 1), heads_of(qkv, 2))
    x = lin(a, p.proj) * p.ls1 + p.x
    f = torch.from_numpy(gelu_fast32(lin(layernorm_any(x, *p.n2, torch.float32), p.fc1).numpy()))
    return lin(f, p.fc2) * p.ls2 + x


def block_tol():
    """4 x max|emulation - float64|: what the emulation cannot reproduce is the MFMAs' summation order, the online rescaling across key tiles
    and v_exp_f32 / v_rcp_f32 at 1 ulp"""
    return 4 * float((block_emulation().double() - block64()).abs().max())


def test_vit_block_on_the_production_chain(P):
    """layernorm_ss -> gemm_ss_qkv -> attention_qkv_ss(out_ss) -> gemm_ss(proj, gamma, res, in place) -> layernorm_ss -> gemm_ss(fc1, GELU, out_ss)
    -> gemm_ss(fc2, gamma, res, in place), exactly as dav2.py chains them, against the block in float64.  The emulation's error is 2.3e-5 at
    max|ref| 5.0 (tolerance 9.0e-5), of which the kernels use 0.30 on an MI355X: 1.2 x the emulation's own error"""
    p = block_inputs()
    M, D = p.x.shape
    dev = lambda t: t.to(DEV)  # noqa: E731
    pack = lambda wb: P.pack_conv(dev(wb[0]), dev(wb[1]), prec=PREC_BF16X3)  # noqa: E731
    x, h = dev(p.x).clone(), torch.full((M, D), NAN, device=DEV)
    P.layernorm_ss(x, M, D, D, dev(p.n1[0]), dev(p.n1[1]), LN_EPS, h)
    a = P.attention_qkv_ss(P.gemm_ss_qkv(h, pack(p.qkv), BLOCK.heads), BLOCK.B, BLOCK.N, BLOCK.heads)
    P.gemm_ss(a, pack(p.proj), out=x, gamma=dev(p.ls1), res=x)
    P.layernorm_ss(x, M, D, D, dev(p.n2[0]), dev(p.n2[1]), LN_EPS, h)
    f = P.gemm_ss(h, pack(p.fc1), act=ACT_GELU, out_ss=True)
    P.gemm_ss(f, pack(p.fc2), out=x, gamma=dev(p.ls2), res=x)
    print(f"[vit] f block: emulation error {block_tol() / 4:.3e}, max|ref| {float(block64().abs().max()):.3f}")
    within(x, block64(), block_tol(), "f ViT block")
