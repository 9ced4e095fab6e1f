"""GPU parity, per pixel and channel, of the two fp16 + block-scaled-fp6 kernels of csrc/conv3x3_f6.hip -- conv3x3_c256_f6_kernel (ops.conv3x3_f6: the
persistent GatedConvUnit conv + skip) and conv3x3_c256_gate_f6_kernel<X2IN> (ops.conv3x3_ln_gate_f6: the unit's tail) -- against the host emulation of
their documented arithmetic (tests/f6_emulation.py) and against plain float64, at the smallest shapes that reach every edge of tile, superslab, tile
walk, slice and block scale.

Every row is explicit (no seeded sweep) and names the kernel it expects; nothing sets a dispatch switch or an environment variable, so the persistent
grid is the literal 256.  Operands are built by hand: a source slice sits in a buffer that is NaN outside the slice, a destination is NaN where the op
must write and SENTINEL in every other channel (asserted bit-identical afterwards), res and pre are slices of buffers with a pixel stride above 256
that are NaN outside.  Every row also asserts the range word bit for bit (max |relu?(x) x_scale|).

Criterion, every comparison: max |got - ref| / max(1, max |ref|), printed as a share of its bar, then asserted.  No bar comes from the kernels:
  conv against the emulation E:         S_row / 3   (S_row: the max-norm distance between E and ``exact`` on that row's data -- the
                                                     ``err * 3 < scheme`` rule of test_conv3x3_f6_matches_the_documented_arithmetic per pixel and row)
  conv against ``exact``:               4 x S_row
  gate tail against the emulated graph: 2e-5        (TOL of tests/test_gate_tail_gpu.py: everything behind the conv is that file's bf16x3 epilogue)
  gate tail against ``exact``:          4 x the emulated graph's own distance from ``exact``
  the tie row, the range words, the X2 split and the taps row: exact.
EMU holds (S_row, A_row) per conv row (A_row: E against the same terms accumulated in float32 in the kernel's order -- how much of the bar fp32
accumulation uses) and the emulated graph's distance per tail row; tests/test_f6_kernels_host.py recomputes them and checks the rows' claims, the
planted data and the discrimination of the references without a GPU.

What the rows found: no row found a kernel wrong, and no kernel was changed.  The tie row comes back with error 0 against the ties-to-even emulation
(the lower-neighbour rule of tools/studies/split_arith_study.py would be off by 2^-15 there): the instruction rounds ties to the even code, as
tests/test_conv3x3_f6.py says.  Every range word, the X2 split and the taps row are exact; every sentinel is untouched.
Planted mutations (on a scratch copy of csrc/conv3x3_f6.hip in a scratch library, not committed; values only, no address or bound moved), each run once
against this file (73 cases) and once against tests/test_conv3x3_f6.py (31 cases):
  (A) the residual block x - f16 x converted, and its scale stored, with the q6(x) block's E8M0 code: 68 cases of this file fail -- every conv and tail
      row, the tie row and the taps row; f16exact (a zero residual has no scale), the range-word and the repeat tests pass, as they must.  28 of 31 earlier
      cases fail too (all but the X2-output test and two range-guard cases): a dropped correction of EVERY pixel is well above the rel-L2 bars.
  (B) the halo pixels converted by waves 4 .. 7 skip the input ReLU: 34 cases fail -- every conv row with relu_in, negative inputs and an image under halo
      rows 5 .. 9; the rows that pass are the ones that must: no ReLU, non-negative data (the edge rows), h <= 2 (g-1x1x16, w257-*, w514-*: those halo rows
      lie outside the image) and every tail row (no input ReLU in that kernel).  14 earlier cases fail (the relu_in half of test_conv3x3_f6_vs_fp64, the
      documented-arithmetic test, the networks).
  (C) stage-1 epilogue: b1 loaded from c0 instead of c0 + 4: 44 cases fail -- every conv row with a bias, none without (nobias, bare, wscale-up, tie) and
      no tail row (another epilogue).  12 earlier cases fail (the biased half of test_conv3x3_f6_vs_fp64, heavy-tailed, documented-arithmetic, two network cases).
So the earlier file was blind to none of the three -- each of them touches every pixel; what it could not see is an error confined to a few pixels (a halo
row of one tile, one workgroup's second tile, one block scale), which is what the per-pixel bars, the walk rows and the planted data above are for;
tests/test_f6_kernels_host.py plants each such error in the emulation: the smallest move on any row that claims the edge is 18 x the bar (the
residual-scale error on rng-last); a stale first superslab moves a walked tile by 5e4 .. 8e4 x the bar.

Largest err / bar on an MI355X (73 cases, 7 s): conv against the emulation 0.22 (c512; c256 0.19, the one-superslab rows 0.14), against ``exact`` 0.25
(g-1x24x48); tail against the emulated graph 0.13 (t-bare-f32), against ``exact`` 0.37 (t-xs-f32-end); taps row against the emulated graph 0.08; tie row 0.
"""
import collections
import functools
import math
import zlib

import numpy as np
import pytest
import torch

import f6_emulation as E

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENTINEL = -7.5
TAIL_TOL = 2e-5      # tests/test_gate_tail_gpu.py::TOL
S_MAX = 2e-5         # no row's data may put the arithmetic itself further than this from float64
K_CONV = "conv3x3_c256_f6_kernel<256,f16f6>"
K_TAIL = "conv3x3_c256_gate_f6_kernel<256,f16f6>"
COUT = 256


@pytest.fixture(scope="module")
def P():
    from patchrefinerv2_amd import ops
    ops.L.load()
    return ops


def last_kernel(P) -> str:
    return P.L.load().prv2_last_kernel().decode()


def seed_of(row_id, k):
    return zlib.crc32(row_id.encode()) % (2 ** 30) + k


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy()


def share(got, ref, bar, what):
    """max |got - ref| / max(1, max |ref|) as a share of ``bar``: printed, then asserted"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite output"
    err = float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))
    s = err / bar if bar > 0 else (0.0 if err == 0 else math.inf)
    print(f"SHARE {what}: err / bar = {s:.3f} of {bar:.3g}")
    assert s <= 1.0, f"{what}: err {err:.3e} is {s:.3f} of the bar {bar:.3e}"
    return s


# ---- rows ------------------------------------------------------------------------------------------------------------------------------------------
# xs / ys / rs / ps = (first channel, pixel stride) of the source / destination / res / pre slice; x_log2: the caller's x_scale; w_log2: the weights
# are multiplied by 2^w_log2 (moves the packed weight scale); data: see conv_inputs
Row = collections.namedtuple("Row", "id n h w cin o")
CONV_DEFAULTS = dict(relu_in=True, bias=True, res=True, xs=None, ys=(8, 272), rs=(4, 264), x2out=False, x_log2=0, w_log2=0, data="randn")
TAIL_DEFAULTS = dict(x2=True, pre=True, res=True, act="relu", gate_bias=True, ln_eps=1e-6, xs=None, ys=(8, 272), rs=(4, 264), ps=(8, 276), taps=False)


def R(id_, n, h, w, cin, **o):
    assert set(o) <= set(CONV_DEFAULTS), o
    return Row(id_, n, h, w, cin, tuple(sorted(o.items())))


def T(id_, n, h, w, cin, **o):
    assert set(o) <= set(TAIL_DEFAULTS), o
    return Row(id_, n, h, w, cin, tuple(sorted(o.items())))


def opts(row):
    return dict(TAIL_DEFAULTS if row.id.startswith("t-") else CONV_DEFAULTS, **dict(row.o))


S917 = (1, 9, 17)   # four ragged tiles
GEOMETRY = [
    R("g-1x1x16", 1, 1, 16, 64),          # both halo rows outside the image
    R("g-1x8x16", 1, 8, 16, 64),          # exactly one tile
    R("g-1x9x17", *S917, 64),             # four ragged tiles, one superslab: the first is also the last
    R("g-1x7x31", 1, 7, 31, 64),
    R("g-1x16x32", 1, 16, 32, 64),        # tile corners meet inside the image
    R("g-1x24x48", 1, 24, 48, 64),        # 9 tiles: the middle one has its whole halo inside the image
    R("g-1x24x48-c192", 1, 24, 48, 192),
    R("g-1x7x97", 1, 7, 97, 64),          # 7 tiles
    R("g-2x9x17", 2, 9, 17, 64),          # 8 tiles; image 1's top halo / image 0's bottom halo read zero, not the other image
    R("g-2x9x17-c128", 2, 9, 17, 128),
    R("edge-1x9x17", *S917, 64, data="edges"),     # large values in the edge columns: a halo pixel taken from the linear-memory neighbour shows at full size
    R("edge-2x8x16", 2, 8, 16, 128, data="edges"),  # ... and in the rows next to the other image
]
CHANNELS = [R(f"c{c}", *S917, c) for c in (128, 192, 256, 512)] + [R("c192-norelu", *S917, 192, relu_in=False)]   # 2, 3, 4, 8 superslabs (1: g-1x9x17)
SLICES = [
    R("xs-end", *S917, 64, xs=(64, 128)),          # the source slice ends at the last channel of its buffer: the record bound of the last pixel
    R("xs-mid", *S917, 128, xs=(8, 144)),          # ... and one that does not
    R("xs-end-c192", 2, 9, 17, 192, xs=(64, 256)),
    R("y-dense", *S917, 64, ys=None),
    R("y-slice-4", *S917, 64, ys=(4, 268)),
    R("res-dense", *S917, 64, rs=(0, 256)),
    R("nores", *S917, 64, res=False),
    R("nobias", *S917, 64, bias=False),
    R("bare", *S917, 128, res=False, bias=False, relu_in=False),
    R("norelu", *S917, 64, relu_in=False),
    R("x2out", *S917, 64, x2out=True),
    R("x2out-c128-nores", 2, 9, 17, 128, x2out=True, res=False),
]
WALK = [   # tile counts 1, 7, 8, 9: the geometry rows.  > 256 and > 512 tiles: workgroups walk two and three tiles
    R("w257-c64", 1, 2, 4097, 64), R("w257-c192", 1, 2, 4097, 192),
    R("w514-c64", 1, 1, 8209, 64), R("w514-c192", 1, 1, 8209, 192),
    R("wimg-c64", 65, 9, 17, 64), R("wimg-c192", 65, 9, 17, 192),    # 4 tiles per image: a workgroup's consecutive tiles lie in different images
]
SCALES = [
    R("xscale-up", *S917, 64, x_log2=5), R("xscale-down", *S917, 128, x_log2=-6, relu_in=False),
    R("wscale-down", *S917, 64, w_log2=6), R("wscale-up", *S917, 64, w_log2=-5, x_log2=3, res=False, bias=False),
    R("rng-00", *S917, 64, data="max00"), R("rng-last", *S917, 64, data="maxlast"), R("rng-blk", *S917, 128, data="maxblk", relu_in=False),
]
BLOCKS = [
    R("zero-block", *S917, 64, data="zeroblk"),          # an all-zero block and one that is all negative under the ReLU
    R("zero-block-c128-norelu", *S917, 128, data="zeroblk", relu_in=False),
    R("outlier", *S917, 64, data="outlier"),             # one element 2^12 times the rest of its block
    R("pow2", *S917, 64, data="pow2"),                   # block maxima exactly 4 and one ulp below
    R("f16exact", *S917, 64, data="f16exact"),           # the residual block is all zero
]
TIE = R("tie", *S917, 64, data="tie", bias=False, res=False)
CONV_ROWS = GEOMETRY + CHANNELS + SLICES + WALK + SCALES + BLOCKS
RANGE_IDS = ["rng-00", "rng-last", "rng-blk"]

TAIL_ROWS = [
    T("t-x2-256", *S917, 256),                            # the unit's ``out``, mul = the same buffer
    T("t-f32-512", *S917, 512, x2=False),                 # the concat form, mul = its first half
    T("t-x2-512", *S917, 512),
    T("t-f32-256", *S917, 256, x2=False),
    T("t-nopre", *S917, 256, pre=False), T("t-nores", *S917, 256, res=False), T("t-noact", *S917, 256, act="none"),
    T("t-nogb", *S917, 256, gate_bias=False), T("t-eps", *S917, 256, ln_eps=1e-2), T("t-bare-f32", *S917, 256, x2=False, pre=False, res=False),
    T("t-xs", *S917, 256, xs=(8, 272)), T("t-xs-f32-end", *S917, 256, x2=False, xs=(16, 272)),
    T("t-1x1x16", 1, 1, 16, 256), T("t-1x8x16", 1, 8, 16, 256), T("t-1x7x31", 1, 7, 31, 256), T("t-1x16x32", 1, 16, 32, 256),
    T("t-1x7x97", 1, 7, 97, 256),                         # 7 tiles: every block in the remainder branch
    T("t-2x9x17", 2, 9, 17, 256),                         # 8: no remainder
    T("t-1x24x48", 1, 24, 48, 256),                       # 9: r = 1
    T("t-1x17x65", 1, 17, 65, 256, x2=False),             # 15: q = 1, r = 7
]
TAPS = T("t-taps", 3, 20, 24, 256, taps=True, pre=False)
ALL_ROWS = CONV_ROWS + [TIE] + TAIL_ROWS + [TAPS]
ROW_BY_ID = {r.id: r for r in ALL_ROWS}


# ---- data and references -------------------------------------------------------------------------------------------------------------------------------

TIE_UNIT = 2.0 ** -14                                                  # the residual blocks' scale on the tie row
TIE_MIDS = np.concatenate([(E.GRID[:-1] + E.GRID[1:]) / 2, [7.5]])     # the 31 midpoints between neighbouring e2m3 magnitudes, and the largest magnitude
TIE_TAPS = [(1, 1), (1, 0), (0, 1), (2, 2)]                            # (ky, kx) of output channels 64 j .. 64 j + 63


def tie_x(n, h, w, cin):
    """x = 1.5 +- m 2^-14, m running over the e2m3 midpoints, rolled and signed differently per pixel and block: f16 x = 1.5, x - f16 x on exact ties"""
    p = np.arange(n * h * w).reshape(n, h, w, 1, 1)
    b = np.arange(cin // 32).reshape(1, 1, 1, -1, 1)
    i = np.arange(32).reshape(1, 1, 1, 1, 32)
    m = TIE_MIDS[(i + p + 5 * b) % 32]
    sign = np.where((i + p // 3 + b) % 2 == 0, 1.0, -1.0)
    return (1.5 + sign * m * TIE_UNIT).reshape(n, h, w, cin).astype(np.float32)


def tie_w(cin):
    """fp16-exact and one-hot per output channel: channel co takes input channel co % 64 at tap TIE_TAPS[co // 64] with weight 1"""
    w = np.zeros((COUT, cin, 3, 3), dtype=np.float32)
    for co in range(COUT):
        ky, kx = TIE_TAPS[co // 64]
        w[co, co % 64, ky, kx] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def conv_inputs(row):
    """CPU fp32 operands of a conv row (NHWC x / res, PyTorch weights), made once and never written again"""
    o = opts(row)
    n, h, w, cin = row.n, row.h, row.w, row.cin
    sd = lambda k: seed_of(row.id, k)  # noqa: E731
    x = rnd(sd(1), n, h, w, cin) * np.exp(0.5 * rnd(sd(2), n, h, w, 1))    # (per-pixel magnitudes; negative inputs for the ReLU)
    kind = o["data"]
    if kind == "edges":
        x[:, :, 0] *= 32.0
        x[:, :, -1] *= 32.0
        x[:, 0] *= 16.0
        x[:, -1] *= 16.0
        x = np.abs(x)                                                       # (the ReLU keeps all of it)
    elif kind == "zeroblk":
        x[:, :, 1::2, 32:64] = 0.0                                          # an all-zero block in every second column
        x[:, :, 0::3, 0:32] = -np.abs(x[:, :, 0::3, 0:32]) - 0.01           # all negative: zero under the ReLU
    elif kind == "outlier":
        x = x * 2.0 ** -6
        rest = np.abs(x.reshape(n, h, w, -1, 32)).mean(-1)
        x[..., 7::32] = np.where(x[..., 7::32] < 0, -1.0, 1.0) * 2.0 ** 12 * rest   # element 7 of every block: 2^12 times the (mean magnitude of the) rest
        x[..., 7] = np.abs(x[..., 7])                                       # (block 0's survives the ReLU everywhere)
    elif kind == "pow2":
        x = np.clip(x, -3.0, 3.0)
        x[..., 3] = 4.0                                                     # block 0: the maximum is exactly 2^2
        x[..., 40] = np.nextafter(np.float32(4.0), np.float32(0.0))         # block 1: one ulp below
    elif kind == "f16exact":
        x = x.astype(np.float16).astype(np.float32)
    elif kind in ("max00", "maxlast", "maxblk"):
        x = np.clip(x, -30.0, 30.0)
        if kind == "max00":
            x[0, 0, 0, 5] = 37.5
        elif kind == "maxlast":
            x[0, h - 1, w - 1, 33] = 37.5                                   # the last pixel: the one live pixel of the last ragged tile
        else:
            x[0, 4, 9, cin - 1] = -37.5                                     # the last channel of the last 32-channel block (no ReLU on this row)
    elif kind == "tie":
        return dict(x=tie_x(n, h, w, cin), w=tie_w(cin), b=None, res=None)
    else:
        assert kind == "randn", kind
    wt = rnd(sd(3), COUT, cin, 3, 3) / math.sqrt(9 * cin) * 2.0 ** o["w_log2"]
    d = dict(x=np.ascontiguousarray(x, dtype=np.float32), w=wt.astype(np.float32), b=(0.5 * rnd(sd(4), COUT)).astype(np.float32),
             res=rnd(sd(5), n, h, w, COUT).astype(np.float32))
    for v in d.values():
        v.setflags(write=False)
    return d


def conv_finish(y, row):
    d, o = conv_inputs(row), opts(row)
    if o["bias"]:
        y = y + d["b"].astype(np.float64)
    if o["res"]:
        y = y + d["res"].astype(np.float64)
    return y


@functools.lru_cache(maxsize=None)
def conv_emulation(row):
    d, o = conv_inputs(row), opts(row)
    return conv_finish(E.conv(d["x"], d["w"], o["relu_in"], 2.0 ** o["x_log2"]), row)


@functools.lru_cache(maxsize=None)
def conv_exact(row):
    d, o = conv_inputs(row), opts(row)
    return conv_finish(E.exact(d["x"], d["w"], o["relu_in"]), row)


def distance(a, ref):
    return float(np.abs(a - ref).max()) / max(1.0, float(np.abs(ref).max()))


def scheme_error(row):
    """S_row"""
    return distance(conv_emulation(row), conv_exact(row))


def accumulation_error(row):
    """A_row"""
    d, o = conv_inputs(row), opts(row)
    y = E.conv_f32(d["x"], d["w"], o["relu_in"], 2.0 ** o["x_log2"])
    if o["bias"]:
        y = y + d["b"]
    if o["res"]:
        y = y + d["res"]
    assert y.dtype == np.float32
    return distance(y.astype(np.float64), conv_emulation(row))


@functools.lru_cache(maxsize=None)
def tail_inputs(row):
    o = opts(row)
    n, h, w, cin = row.n, row.h, row.w, row.cin
    sd = lambda k: seed_of(row.id, k)  # noqa: E731
    x = rnd(sd(1), n, h, w, cin).astype(np.float32)
    if o["x2"]:
        x = E.x2_value(x)                                                   # a pre-split buffer holds exactly hi + lo
    d = dict(x=x, w=(rnd(sd(2), COUT, cin, 3, 3) / math.sqrt(9 * cin)).astype(np.float32), b=(0.5 * rnd(sd(3), COUT)).astype(np.float32),
             lnw=(1 + 0.2 * rnd(sd(4), COUT)).astype(np.float32), lnb=(0.1 * rnd(sd(5), COUT)).astype(np.float32),
             gw=(rnd(sd(6), COUT, COUT) / 16.0).astype(np.float32), gb=(0.5 * rnd(sd(7), COUT)).astype(np.float32),
             res=rnd(sd(8), n, h, w, COUT).astype(np.float32), pre=(0.5 * rnd(sd(9), n, h, w, COUT)).astype(np.float32))
    for v in d.values():
        v.setflags(write=False)
    return d


def tail_finish(y, row, pre=None):
    d, o = tail_inputs(row), opts(row)
    pre = d["pre"] if o["pre"] else pre
    return E.gate_tail(y, d["b"], pre, d["lnw"], d["lnb"], o["ln_eps"], o["act"], d["gw"], d["gb"] if o["gate_bias"] else None, d["x"][..., :COUT],
                       d["res"] if o["res"] else None)


@functools.lru_cache(maxsize=None)
def tail_emulation(row):
    d = tail_inputs(row)
    return tail_finish(E.conv(d["x"], d["w"]), row)


@functools.lru_cache(maxsize=None)
def tail_exact(row):
    d = tail_inputs(row)
    return tail_finish(E.exact(d["x"], d["w"]), row)


def graph_error(row):
    return distance(tail_emulation(row), tail_exact(row))


# (S_row, A_row) of the conv rows; the emulated graph's distance from ``exact`` of the tail rows -- measured on the CPU, recomputed by the host file
EMU = {
    "g-1x1x16": (5.573e-06, 5.923e-08), "g-1x8x16": (9.683e-06, 1.631e-07), "g-1x9x17": (8.927e-06, 1.745e-07), "g-1x7x31": (8.996e-06, 1.081e-07),
    "g-1x16x32": (9.328e-06, 1.615e-07), "g-1x24x48": (9.414e-06, 1.580e-07), "g-1x24x48-c192": (9.506e-06, 2.543e-07),
    "g-1x7x97": (1.137e-05, 1.922e-07), "g-2x9x17": (1.081e-05, 1.387e-07), "g-2x9x17-c128": (9.525e-06, 2.381e-07),
    "edge-1x9x17": (1.444e-05, 1.847e-07), "edge-2x8x16": (1.278e-05, 2.430e-07), "c128": (8.850e-06, 2.095e-07), "c192": (1.012e-05, 2.076e-07),
    "c256": (9.218e-06, 2.499e-07), "c512": (9.118e-06, 4.164e-07), "c192-norelu": (1.033e-05, 1.943e-07), "xs-end": (9.083e-06, 1.406e-07),
    "xs-mid": (8.230e-06, 2.062e-07), "xs-end-c192": (9.800e-06, 2.235e-07), "y-dense": (1.261e-05, 1.436e-07), "y-slice-4": (7.476e-06, 1.202e-07),
    "res-dense": (1.046e-05, 1.491e-07), "nores": (1.083e-05, 1.791e-07), "nobias": (1.141e-05, 1.277e-07), "bare": (1.238e-05, 2.779e-07),
    "norelu": (9.794e-06, 1.853e-07), "x2out": (7.869e-06, 1.222e-07), "x2out-c128-nores": (9.261e-06, 2.037e-07), "w257-c64": (1.599e-05, 2.135e-07),
    "w257-c192": (1.348e-05, 3.156e-07), "w514-c64": (1.020e-05, 1.064e-07), "w514-c192": (9.292e-06, 1.693e-07), "wimg-c64": (1.596e-05, 2.127e-07),
    "wimg-c192": (1.076e-05, 2.421e-07), "xscale-up": (9.168e-06, 1.358e-07), "xscale-down": (1.143e-05, 2.233e-07),
    "wscale-down": (1.491e-05, 2.096e-07), "wscale-up": (1.628e-06, 2.538e-08), "rng-00": (1.747e-05, 2.299e-07), "rng-last": (1.669e-05, 1.089e-07),
    "rng-blk": (1.362e-05, 2.140e-07), "zero-block": (7.684e-06, 1.040e-07), "zero-block-c128-norelu": (1.070e-05, 1.671e-07),
    "outlier": (1.837e-05, 2.505e-07), "pow2": (9.365e-06, 1.432e-07), "f16exact": (6.434e-06, 1.268e-07),
}
EMU_TAIL = {
    "t-x2-256": 2.948e-06, "t-f32-512": 3.355e-06, "t-x2-512": 3.323e-06, "t-f32-256": 3.307e-06, "t-nopre": 3.524e-06, "t-nores": 4.249e-06,
    "t-noact": 5.797e-06, "t-nogb": 3.590e-06, "t-eps": 3.000e-06, "t-bare-f32": 5.919e-06, "t-xs": 2.563e-06, "t-xs-f32-end": 2.531e-06,
    "t-1x1x16": 2.031e-06, "t-1x8x16": 2.889e-06, "t-1x7x31": 2.783e-06, "t-1x16x32": 3.542e-06, "t-1x7x97": 3.023e-06, "t-2x9x17": 3.952e-06,
    "t-1x24x48": 4.004e-06, "t-1x17x65": 3.535e-06,
}


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------------------------

def x2_pack(v):
    """fp32 [..., c] (c % 8 == 0) -> the float32 container of its X2 image: per 8 channels [8 bf16 hi | 8 bf16 lo] (include/prv2.h)"""
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    g = torch.cat([hi.reshape(*v.shape[:-1], -1, 8), lo.reshape(*v.shape[:-1], -1, 8)], -1)
    return g.reshape(*v.shape[:-1], -1).contiguous().view(torch.float32)


def sliced(P, v, sl, x2=False):
    """NHWC numpy -> Feat: channels [c0, c0 + c) of a buffer of pixel stride ld that is NaN everywhere else (sl None: dense)"""
    t = torch.from_numpy(np.array(v))
    if x2:
        t = x2_pack(t)
    c = t.shape[3]
    c0, ld = sl if sl is not None else (0, c)
    buf = torch.full((*t.shape[:3], ld), NAN)
    buf[..., c0:c0 + c] = t
    return P.Feat(buf.to(DEV), c, c0, x2)


def destination(P, row, sl, x2=False):
    c0, ld = sl if sl is not None else (0, COUT)
    buf = torch.full((row.n, row.h, row.w, ld), SENTINEL)
    buf[..., c0:c0 + COUT] = NAN
    return P.Feat(buf.to(DEV), COUT, c0, x2)


def collect(dst, what):
    """the written channels on the CPU; every other channel of the buffer still holds SENTINEL, bit for bit"""
    buf = dst.buf.cpu()
    c0 = dst.c0
    rest = torch.cat([buf[..., :c0], buf[..., c0 + COUT:]], -1).contiguous().view(torch.int32)
    want = torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32)
    assert bool((rest == want).all()), f"{what}: wrote outside its channels"
    return buf[..., c0:c0 + COUT].contiguous()


def dev(v):
    return torch.from_numpy(np.array(v)).to(DEV)   # (a copy: the cached operands are read-only)


def run_conv(P, row, x2out=False):
    """-> (the 256 written channels [n, h, w, 256] on the CPU -- fp32, or the X2 container --, kernel name, range word)"""
    d, o = conv_inputs(row), opts(row)
    cw = P.pack_conv3x3_f6(dev(d["w"]), dev(d["b"]) if o["bias"] else None)
    assert cw.w_scale == E.w_scale_of(d["w"])
    cw.x_scale = 2.0 ** o["x_log2"]
    x = sliced(P, d["x"], o["xs"])
    res = sliced(P, d["res"], o["rs"]) if o["res"] else None
    dst = destination(P, row, o["ys"], x2=x2out)
    assert P.conv3x3_f6_supported(x, COUT, row.cin)
    P.conv3x3_f6(x, cw, dst, relu_in=o["relu_in"], res=res)
    name = last_kernel(P)
    word = int(cw.range.cpu().item()) & 0xFFFFFFFF
    return collect(dst, row.id), name, word


def check_conv(P, row):
    got, name, word = run_conv(P, row)
    assert name == K_CONV, (row.id, name)
    d, o = conv_inputs(row), opts(row)
    assert word == E.range_word(d["x"], o["relu_in"], 2.0 ** o["x_log2"]), (row.id, hex(word))
    s, _ = EMU[row.id]
    assert 0 < s <= S_MAX
    share(got.numpy(), conv_emulation(row), s / 3, f"conv {row.id} vs emulation")
    share(got.numpy(), conv_exact(row), 4 * s, f"conv {row.id} vs exact")
    return got


@pytest.mark.parametrize("row", CONV_ROWS, ids=lambda r: r.id)
def test_conv_rows(P, row):
    got = check_conv(P, row)
    if opts(row)["x2out"]:   # the pre-split output is exactly the bf16 split of the fp32 result of the same call
        got2, name, _ = run_conv(P, row, x2out=True)
        assert name == K_CONV
        assert torch.equal(got2.view(torch.int32), x2_pack(got).view(torch.int32)), row.id


@pytest.mark.parametrize("rid", RANGE_IDS)
def test_range_word_is_the_planted_maximum(P, rid):
    row = ROW_BY_ID[rid]
    _, _, word = run_conv(P, row)
    assert word == int(np.float32(37.5).view(np.uint32)), hex(word)


def test_tie_row_rounds_ties_to_even(P):
    """fp16-exact one-hot weights, residuals x - f16 x exactly on e2m3 midpoints of their block scale: y - 1.5 is q6 of the residual alone, every sum
    exact in fp32.  Expected: error 0 against the emulation (ties to the even code); a quantiser on another tie rule misses by half an fp6 step."""
    got, name, word = run_conv(P, TIE)
    assert name == K_CONV
    d = conv_inputs(TIE)
    assert word == E.range_word(d["x"], True, 1.0)
    ref = conv_emulation(TIE)
    err = float(np.abs(got.numpy().astype(np.float64) - ref).max())
    other = float(np.abs(E.conv(d["x"], d["w"], True, tie="down") - ref).max())
    print(f"SHARE tie row: |kernel - ties-to-even emulation| max = {err:.3e} (the lower-neighbour rule would be off by {other:.3e})")
    assert err == 0.0


def run_tail(P, row, pre_feat=None, taps=None):
    d, o = tail_inputs(row), opts(row)
    cw = P.pack_conv3x3_f6(dev(d["w"]), dev(d["b"]))
    x = sliced(P, d["x"], o["xs"], x2=o["x2"])
    mul = x.slice(0, COUT)
    res = sliced(P, d["res"], o["rs"]) if o["res"] else None
    pre = sliced(P, d["pre"], o["ps"]) if o["pre"] else pre_feat
    dst = destination(P, row, o["ys"])
    assert P.conv3x3_f6_supported(x, COUT, row.cin, allow_x2=True)
    kw = dict(taps=taps[0], boxes=taps[1], spatial_scale=taps[2]) if taps is not None else {}
    P.conv3x3_ln_gate_f6(x, cw, (dev(d["lnw"]), dev(d["lnb"])), P.pack_gate(dev(d["gw"])), dev(d["gb"]) if o["gate_bias"] else None, dst,
                         act=P.ACT_RELU if o["act"] == "relu" else P.ACT_NONE, mul=mul, res=res, ln_eps=o["ln_eps"], pre=pre,
                         pre_cin=COUT if (pre is not None or taps is not None) else 0, **kw)
    name = last_kernel(P)
    word = int(cw.range.cpu().item()) & 0xFFFFFFFF
    assert word == E.range_word(d["x"], False, 1.0), (row.id, hex(word))
    return collect(dst, row.id), name


@pytest.mark.parametrize("row", TAIL_ROWS, ids=lambda r: r.id)
def test_tail_rows(P, row):
    got, name = run_tail(P, row)
    assert name == K_TAIL, (row.id, name)
    g = EMU_TAIL[row.id]
    assert g > 0
    share(got.numpy(), tail_emulation(row), TAIL_TOL, f"tail {row.id} vs emulated graph")
    share(got.numpy(), tail_exact(row), 4 * g, f"tail {row.id} vs exact")


TAP_SCALE, TAP_MAP, TAP_KNOTS = 0.25, (20, 48), (0.25, 0.5)   # tests/test_taps_fold.py::SHAPES["ragged20x24"]


def test_tail_taps_row(P):
    """prv2_conv3x3_ln_gate_f6_taps against the same call given the materialised ``pre``: bit equality, the bar of tests/test_taps_fold.py -- and that
    pair against the emulated graph with the gathered addend"""
    row = TAPS
    (H, W), (kbh, kbw), h, w = TAP_MAP, TAP_KNOTS, row.h, row.w
    bh, bw, fh, fw = kbh * h / TAP_SCALE, kbw * w / TAP_SCALE, H / TAP_SCALE, W / TAP_SCALE
    org = [(0.0, 0.0), (fw - bw, fh - bh), (0.37 * (fw - bw), 0.61 * (fh - bh))]
    boxes = torch.tensor([[x, y, x + bw, y + bh] for x, y in org], dtype=torch.float32, device=DEV)
    taps = P.CoarseTaps(P.Feat(dev(0.2 * rnd(seed_of(row.id, 20), 1, H, W, 9 * COUT))), COUT, TAP_KNOTS)
    pre = taps.gather(boxes, TAP_SCALE, h, w)
    folded, k1 = run_tail(P, row, taps=(taps, boxes, TAP_SCALE))
    given, k2 = run_tail(P, row, pre_feat=pre)
    bare, _ = run_tail(P, row)
    assert k1 == k2 == K_TAIL
    assert not torch.equal(given, bare)
    assert torch.equal(folded, given), int((folded != given).sum())
    d = tail_inputs(row)
    ref = tail_finish(E.conv(d["x"], d["w"]), row, pre=pre.buf[..., pre.c0:pre.c0 + COUT].cpu().numpy())
    share(given.numpy(), ref, TAIL_TOL, "tail t-taps vs emulated graph")


def test_second_call_is_bit_equal(P):
    for rid in ("w514-c192", "wimg-c64", "g-1x24x48-c192"):
        a, b = run_conv(P, ROW_BY_ID[rid])[0], run_conv(P, ROW_BY_ID[rid])[0]
        assert torch.equal(a, b), rid
