"""Host emulation (numpy float64) of the fp16 + block-scaled-fp6 arithmetic of csrc/conv3x3_f6.hip, as include/prv2.h and the head of that
file document it -- a plain helper module for tests/test_f6_kernels_gpu.py and tests/test_f6_kernels_host.py (no fixtures, nothing loads the library):

    x w  ~=  f16(x') f16(w')  +  q6(x') q6(w' - f16 w')  +  q6(x' - f16 x') q6(w')        x' = relu?(x) x_scale,  w' = w w_scale,  result x out_scale

* f16: round to nearest even, x' clamped to +-65504 first (the loader's v_med3), w' not (|w'| < 2);
* q6: fp6 e2m3 with one power-of-two scale per 32 consecutive channels.  The scale's E8M0 code is the block maximum's biased fp32 exponent - 2,
  clamped to [1, 254] (e8m0_of): 2^(floor(log2 max) - 2) for every normal maximum, 2^-126 for an all-zero block.  Elements are rounded to the nearest
  of the 32 magnitudes, TIES TO THE EVEN CODE, and saturate at 7.5 (v_cvt_scalef32_2xpk16_fp6_f32).  The quantiser is built here from the 64 codes;
  tools/studies/split_arith_study.py::mx_quant takes the lower neighbour on ties and is only compared with (tie="down");
* products and sums exact in float64 (``conv``); ``conv_f32``: the same terms accumulated in float32 in the kernel's order (superslab, tap, fp16 slab 0,
  fp16 slab 1, the K = 128 fp6 product), each matrix instruction's dot product exact -- it says how much of a bar the fp32 accumulation uses.

Around the conv, the GatedConvUnit tail in float64, written out (``gate_tail``), and ``exact``: the conv as plain float64 F.conv2d.
Arrays are NHWC; weights are PyTorch [cout, cin, 3, 3]."""
import numpy as np
import torch

BLOCK = 32         # channels per E8M0 scale
SUPERSLAB = 64     # channels per main-loop step
TH, TW = 8, 16     # the tile


# ---- fp6 e2m3 ----------------------------------------------------------------------------------------------------------------------------------

def e2m3_decode(code):
    """the value of a 6-bit e2m3 code: sign (bit 5), 2 exponent bits (bias 1), 3 mantissa bits; exponent 0 is subnormal"""
    code = int(code)
    s, e, m = (code >> 5) & 1, (code >> 3) & 3, code & 7
    v = m / 8.0 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1)
    return -v if s else v


E2M3_VALUES = np.array([e2m3_decode(c) for c in range(64)])
GRID = E2M3_VALUES[:32]          # the 32 magnitudes, ascending: index == code
E2M3_MAX = float(GRID[-1])       # 7.5


def e8m0_of(m):
    """E8M0 code of a block with maximum magnitude m (fp32): biased exponent - 2, clamped to [1, 254]"""
    eb = (np.asarray(m, dtype=np.float32).view(np.uint32) >> 23) & 0xFF
    return np.clip(eb.astype(np.int64) - 2, 1, 254)


def round_e2m3(a, tie="even"):
    """magnitudes a >= 0 (in units of the block scale) -> the nearest e2m3 magnitude; ties: "even" (the even code), "down", "up"; saturating"""
    a = np.asarray(a, dtype=np.float64)
    idx = np.clip(np.searchsorted(GRID, a, side="left"), 1, 31)
    lo, hi = GRID[idx - 1], GRID[idx]
    dlo, dhi = a - lo, hi - a
    tie_hi = {"even": idx % 2 == 0, "down": np.zeros_like(idx, dtype=bool), "up": np.ones_like(idx, dtype=bool)}[tie]
    q = np.where((dhi < dlo) | ((dhi == dlo) & tie_hi), hi, lo)
    return np.where(a >= E2M3_MAX, E2M3_MAX, q)


def block_codes(v):
    """E8M0 codes of the 32-channel blocks of v [..., c]: shape [..., c / 32]"""
    assert v.shape[-1] % BLOCK == 0
    m = np.abs(v.reshape(*v.shape[:-1], -1, BLOCK)).max(-1)
    assert np.array_equal(m.astype(np.float32).astype(np.float64), m), "block maxima are fp32 values"
    return e8m0_of(m)


def q6(v, tie="even", codes=None):
    """block-scaled e2m3 of v [..., c] (fp32 values held in float64) along the last axis; codes: E8M0 codes to use instead of the blocks' own"""
    v = np.asarray(v, dtype=np.float64)
    codes = block_codes(v) if codes is None else codes
    sc = np.repeat(2.0 ** (codes.astype(np.float64) - 127.0), BLOCK, axis=-1)
    return np.sign(v) * round_e2m3(np.abs(v) / sc, tie) * sc


def f16(v, clamp=True):
    v = np.asarray(v, dtype=np.float64)
    if clamp:
        v = np.clip(v, -65504.0, 65504.0)
    return v.astype(np.float16).astype(np.float64)


# ---- operand splits -------------------------------------------------------------------------------------------------------------------------------

def scaled_input(x, relu_in, x_scale):
    """x' = relu?(x) x_scale as the loader forms it in fp32 (x_scale a power of two)"""
    x = np.asarray(x, dtype=np.float32)
    xs = (np.maximum(x, np.float32(0)) if relu_in else x) * np.float32(x_scale)
    return xs.astype(np.float64)


def range_word(x, relu_in, x_scale):
    """what the kernel leaves in its range word: the float32 bits of max |x'|"""
    return int(np.abs(scaled_input(x, relu_in, x_scale)).max().astype(np.float32).view(np.uint32))


def split_x(x, relu_in=False, x_scale=1.0, tie="even", resid_codes="own"):
    """-> (f16 x', q6 x', q6(x' - f16 x')), NHWC float64.  resid_codes="main": the planted error of quantising the residual with q6(x')'s scales"""
    xs = scaled_input(x, relu_in, x_scale)
    xh = f16(xs)
    r = xs - xh
    return xh, q6(xs, tie), q6(r, tie, codes=block_codes(xs) if resid_codes == "main" else None)


def split_w(w, w_scale, tie="even"):
    """PyTorch [cout, cin, 3, 3] -> (f16 w', q6(w' - f16 w'), q6 w') as [cout, 3, 3, cin] float64: the part each of split_x's meets"""
    ws = (np.asarray(w, dtype=np.float32) * np.float32(w_scale)).astype(np.float64).transpose(0, 2, 3, 1)
    wh = f16(ws, clamp=False)
    return wh, q6(ws - wh, tie), q6(ws, tie)


def w_scale_of(w):
    """ops.pack_conv3x3_f6's power of two: max |w w_scale| in [1, 2)"""
    amax = float(np.abs(np.asarray(w, dtype=np.float32)).max())
    return 2.0 ** -int(np.floor(np.log2(amax))) if amax > 0 else 1.0


# ---- the conv ----------------------------------------------------------------------------------------------------------------------------------------

def pad_zero(p):
    """[n, h, w, c] -> [n, h + 2, w + 2, c] with the zero halo of a pad-1 conv"""
    return np.pad(p, ((0, 0), (1, 1), (1, 1), (0, 0)))


def pad_linear(p, axis):
    """the planted halo error: outside the image the halo takes its neighbour in LINEAR MEMORY instead of zero.  axis "x": left of column 0 the previous
    row's last pixel, right of the last column the next row's first; axis "y": above image i the last row of image i - 1, below it the first of image i + 1"""
    out = pad_zero(p)
    if axis == "x":
        out[:, 2:-1, 0] = p[:, :-1, -1]
        out[:, 1:-2, -1] = p[:, 1:, 0]
    else:
        assert axis == "y"
        out[1:, 0, 1:-1] = p[:-1, -1]
        out[:-1, -1, 1:-1] = p[1:, 0]
    return out


def conv_valid(xp_parts, w_parts):
    """sum over the parts of the valid 3x3 correlation of padded [n, h + 2, w + 2, c] with [cout, 3, 3, c]; exact products, float64 sums"""
    X, W = np.concatenate(xp_parts, -1), np.concatenate(w_parts, -1)
    n, hp, wp, k = X.shape
    h, w = hp - 2, wp - 2
    y = np.zeros((n * h * w, W.shape[0]))
    for ky in range(3):
        for kx in range(3):
            y += X[:, ky:ky + h, kx:kx + w].reshape(-1, k) @ np.ascontiguousarray(W[:, ky, kx].T)
    return y.reshape(n, h, w, -1)


def conv(x, w, relu_in=False, x_scale=1.0, w_scale=None, tie="even", swap=False, resid_codes="own", pad=pad_zero):
    """the emulated conv3x3 of x [n, h, w, cin] with w [256, cin, 3, 3], x out_scale, without bias.  swap / resid_codes / pad: planted errors"""
    w_scale = w_scale_of(w) if w_scale is None else w_scale
    xh, qx, qr = split_x(x, relu_in, x_scale, tie, resid_codes)
    wh, qwr, qw = split_w(w, w_scale, tie)
    wp = (wh, qw, qwr) if swap else (wh, qwr, qw)
    return conv_valid([pad(p) for p in (xh, qx, qr)], wp) / (x_scale * w_scale)


def conv_f32(x, w, relu_in=False, x_scale=1.0, w_scale=None):
    """the same terms accumulated in float32 in the kernel's order; x out_scale in float32 -> float32 (the epilogue adds bias and res to it in float32)"""
    w_scale = w_scale_of(w) if w_scale is None else w_scale
    xh, qx, qr = (pad_zero(p) for p in split_x(x, relu_in, x_scale))
    wh, qwr, qw = split_w(w, w_scale)
    n, hp, wp_, c = xh.shape
    h, wd = hp - 2, wp_ - 2
    acc = np.zeros((n * h * wd, wh.shape[0]), dtype=np.float32)
    add = lambda a, t: (a.astype(np.float64) + t).astype(np.float32)  # noqa: E731
    for ss in range(c // SUPERSLAB):
        c0 = ss * SUPERSLAB
        for ky in range(3):
            for kx in range(3):
                win = lambda p, a, b: p[:, ky:ky + h, kx:kx + wd, a:b].reshape(-1, b - a)  # noqa: E731
                wt = lambda p, a, b: np.ascontiguousarray(p[:, ky, kx, a:b].T)  # noqa: E731
                for s in (c0, c0 + BLOCK):
                    acc = add(acc, win(xh, s, s + BLOCK) @ wt(wh, s, s + BLOCK))
                e = c0 + SUPERSLAB
                acc = add(acc, win(qx, c0, e) @ wt(qwr, c0, e) + win(qr, c0, e) @ wt(qw, c0, e))
    out_scale = np.float32(1.0 / (x_scale * w_scale))
    return (acc * out_scale).reshape(n, h, wd, -1)


def exact(x, w, relu_in=False):
    """plain float64 conv3x3 pad 1 (F.conv2d), NHWC in and out, without bias"""
    xv = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64))).permute(0, 3, 1, 2)
    if relu_in:
        xv = torch.relu(xv)
    y = torch.nn.functional.conv2d(xv, torch.from_numpy(np.asarray(w, dtype=np.float64)), None, padding=1)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


# ---- the X2 format and the gate tail -------------------------------------------------------------------------------------------------------------------

def bf16_rne(v):
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32)


def x2_value(v):
    """what an X2 element stands for, and what the gate kernels take of ``mul`` in either format: bf16 hi (RNE) + bf16 lo (RNE of the remainder)"""
    v = np.asarray(v, dtype=np.float32)
    hi = bf16_rne(v)
    return (hi + bf16_rne(v - hi)).astype(np.float32)


def gate_tail(y, bias, pre, lnw, lnb, ln_eps, act, gate_w, gate_b, mul, res):
    """everything behind the conv in float64: + bias, + pre, two-pass LayerNorm over the 256 channels, ReLU or nothing, the 256 x 256 gate (gate_w
    [out, in]) + its bias, sigmoid, x mul (hi + lo of its bf16 split), + res.  y [n, h, w, 256]: the conv without bias"""
    d = lambda t: np.asarray(t, dtype=np.float64)  # noqa: E731
    t = d(y)
    if bias is not None:
        t = t + d(bias)
    if pre is not None:
        t = t + d(pre)
    mu = t.mean(-1, keepdims=True)
    var = ((t - mu) ** 2).mean(-1, keepdims=True)
    t = (t - mu) / np.sqrt(var + ln_eps) * d(lnw) + d(lnb)
    assert act in ("relu", "none")
    if act == "relu":
        t = np.maximum(t, 0.0)
    z = t @ d(gate_w).T
    if gate_b is not None:
        z = z + d(gate_b)
    out = 1.0 / (1.0 + np.exp(-z))
    if mul is not None:
        out = out * d(x2_value(mul))
    if res is not None:
        out = out + d(res)
    return out


# ---- the launch arithmetic of prv2_conv3x3_f6 and of the stage-2 block map, restated -----------------------------------------------------------------

def cdiv(a, b):
    return -(-a // b)


def tile_grid(n, h, w):
    """-> (tiles_x, tiles_y, ntiles)"""
    tx, ty = cdiv(w, TW), cdiv(h, TH)
    return tx, ty, n * tx * ty


def tile_origin(t, n, h, w):
    """tile index -> (image, y0, x0)"""
    tx, ty, _ = tile_grid(n, h, w)
    img, r = divmod(t, tx * ty)
    return img, (r // tx) * TH, (r % tx) * TW


def stage1_walks(ntiles, wgs=256):
    """prv2_conv3x3_f6 + conv3x3_c256_f6_kernel: blocks = min(ceil(ntiles / 8), wgs / 8) * 8 persistent workgroups; workgroup b serves XCD b & 7, whose
    chunk is tiles [xcd * chunk, min((xcd + 1) * chunk, ntiles)), chunk = ceil(ntiles / 8), and walks t_begin = xcd * chunk + (b >> 3), + per, ...
    -> the list of tile sequences, one per workgroup (K = its length)"""
    blocks = min(cdiv(ntiles, 8), wgs // 8) * 8
    per, chunk = max(blocks >> 3, 1), cdiv(ntiles, 8)
    walks = []
    for b in range(blocks):
        xcd, jwg = b & 7, b >> 3
        t_begin, t_end = xcd * chunk + jwg, min((xcd + 1) * chunk, ntiles)
        k = cdiv(t_end - t_begin, per) if t_begin < t_end else 0
        walks.append([t_begin + i * per for i in range(k)])
    return walks


def stage2_tile(b, ntiles):
    """conv3x3_c256_gate_f6_kernel: block b of ntiles -> its tile (XCD b & 7 takes q or q + 1 consecutive tiles)"""
    q, r, xcd = ntiles >> 3, ntiles & 7, b & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (b >> 3)
