"""GPU parity of the PLAIN 3x3 / stride 1 / pad 1 halo kernels -- conv3x3_halo_kernel<32/64/128, f32> (csrc/conv3x3.hip), conv3x3_halo16_kernel /
conv3x3_halo16_narrow_kernel<32/64> in the two bf16 modes with and without the tail step (csrc/conv3x3_m16.hip, every non-GATE, non-UPS instance of
halo16_body), and the f32 remainder strip on igemm_kernel's column window (csrc/igemm.hip) -- against plain float64 on the CPU, through the three
entry points that reach them (ops.conv2d, ops.conv2d_pre, ops.conv2d_tail), at the smallest shapes that cross every edge of tile, slab and channel.

    y = (act(LN_1e-6(conv3x3(relu_in?(x)) + b [+ pre])) * gamma) * mul + res + res2        [| pred1 | pred2 | 0 | 0: conv2d_tail]

Every row is explicit (no seeded sweep) and names the kernel it expects per mode (KERNEL); nothing sets a dispatch switch, so the rows pin the
default ladder.  Sources and destinations are built by hand: a destination is NaN where the op must write and SENTINEL everywhere else (asserted
untouched), the pad channels the 16-byte store path owns are asserted zero, a source slice sits in a buffer that is NaN outside -- except the up
to three channels behind a cin % 4 != 0 slice, which the loader reads (x zero weights) and which hold BIG.

Bars: f32 2e-5 and bf16x3 3e-5 (tests/test_conv_routes_gpu.py::TOL); bf16: 4 x the error of the emulation (the same float64 graph on x and w
rounded to bf16 -- the hi plane of the loader, the hi half of pack_weight_kernel), never above the project's 2e-2, AND 3e-5 against the emulation
itself.  The emulation error of every row is recorded in EMU; tests/test_halo_conv_host.py recomputes it, and checks the tables, the edges they
claim, the references, their discrimination and the feasibility of the bars without a GPU.

What the rows found: no row found a kernel wrong.  One case of the issue cannot run: conv2d_tail at cout 130 -- prv2_conv2d_tail's contract is
cout % 4 == 0 and cout <= 128 (tail_shape_ok), so tiles_n is always 1 there; the row is kept as the documented refusal
(test_conv2d_tail_refuses_more_than_128_channels) and cout 128 is the widest depth-pair row.
Planted mutations (on a scratch copy of csrc/conv3x3_m16.hip, neither committed), each run against this file and against the 18 earlier test
files that reach a conv kernel (853 GPU tests):
  (A) the tail step reading halo buffer (cchunks & 1) ^ 1: 19 cases of this file fail -- every tail-step row of the 128-column kernel, cchunks
      1, 2, 3 and 4 alike, in 8 x 32 and 32 x 8 tiles, with input ReLU, on a source slice and under conv2d_pre, and no other row; the narrow
      kernels' rows (one halo buffer) pass, as they must.  The earlier tests were not blind to it: 51 of them fail (test_hip_ops.py's
      test_conv2d_split_precision / test_conv3x3_remainder_strip on 66 -> 130 and the upsample-fused rows, whose kernel shares the line, and the
      assembled networks); test_conv_routes_gpu.py, test_gate_tail_gpu.py and test_narrow_kernels_gpu.py pass with it.
  (B) jv one block short where cout % 16 != 0 (ceil -> floor): 83 cases fail -- every row whose cout is no multiple of 16 on all three tile widths
      (8, 20, 33, 40, 66, 98, 130, 132, 194; strip tiles, scalar and 16-byte store path, LN over a ragged row, conv2d_pre at 132, conv2d_tail at 8)
      and none with cout % 16 == 0.  59 earlier tests fail with it too (the 130- and 98-column layers of test_hip_ops.py, halo16-128 of
      test_conv_routes_gpu.py, 4 -> 20 of test_narrow_kernels_gpu.py, the networks); cout 8 / 33 / 40 / 194 and the jv == 0 wave half were in no
      earlier test, and test_gate_tail_gpu.py passes (its kernels have no ragged columns).
So neither mutation was missed outright before; what was missing is the row-by-row coverage above, at shapes that take milliseconds.

Largest err / bar on an MI355X (502 cases, 4 s): conv2d f32 0.14, bf16x3 0.23 (both on the offset-40 LayerNorm rows), bf16 0.25 of
4 x the emulation error and 0.08 of 3e-5 against the emulation itself; conv2d_pre bf16x3 0.16, bf16 0.25 / 0.01; conv2d_tail bf16x3 0.17, bf16
0.25 / 0.01 (0.25: the bf16 kernels ARE their emulation); halo against force_generic 0.04 of 2e-5."""
import collections
import functools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")
SENTINEL = -7.5
BIG = 1.0e30          # behind a cin % 4 != 0 slice: read by the loader, multiplied by zero weights
TOL = {"f32": 2e-5, "bf16x3": 3e-5}   # tests/test_conv_routes_gpu.py::TOL
BF16_CAP = 2e-2
BF16_EMU_TOL = 3e-5   # bf16 mode against its own emulation
MODES3 = ("f32", "bf16x3", "bf16")
MODES2 = ("bf16x3", "bf16")

KERNEL = {
    "F32": "conv3x3_halo_kernel<32,f32>", "F64": "conv3x3_halo_kernel<64,f32>", "F128": "conv3x3_halo_kernel<128,f32>",
    "I64": "igemm_kernel<64,f32>", "I128": "igemm_kernel<128,f32>",   # f32 mode, remainder strip: the second launch is the last one
    "H32": "conv3x3_halo16_kernel<32,{}>", "H64": "conv3x3_halo16_kernel<64,{}>", "H128": "conv3x3_halo16_kernel<128,{}>",
}


@pytest.fixture(scope="module")
def P():
    from patchrefinerv2_amd import ops
    ops.L.load()
    return ops


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def roundup(a, b):
    return (a + b - 1) // b * b


def share_of(got, ref, tol):
    """max|got - ref| as a share of the bar tol * max(1, |ref|max)"""
    return float((got.double() - ref.double()).abs().max()) / (tol * max(1.0, float(ref.abs().max())))


def close(got, ref, tol, what):
    got = got.detach().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    s = share_of(got, ref, tol)
    print(f"SHARE {what}: err / tol = {s:.3f} of {tol:g}")
    assert s <= 1.0, f"{what}: max|d| is {s:.3f} of the bar {tol:g} * max(1, |ref|max = {float(ref.abs().max()):.2f})"
    return s


def last_kernel(P) -> str:
    return P.L.load().prv2_last_kernel().decode()


# ---- rows ------------------------------------------------------------------------------------------------------------------------------
# kern = (KERNEL key in f32 mode or None, KERNEL key in the bf16 modes); o: what differs from DEFAULTS
#   xs / ys = (first channel, pixel stride) of the source / destination slice (None: dense, pixel stride roundup(c, 4))
#   wide: mul / res / res2 / pre are slices (first channel 4) of buffers 8 channels wider than roundup(cout, 4)
Row = collections.namedtuple("Row", "id entry n h w cin cout kern o")
DEFAULTS = dict(bias=True, bias_offset=0.0, act="none", relu_in=False, ln=False, gamma=False, mul=False, res=False, res2=False, pre=False,
                xs=None, ys=None, wide=False)
ACTS = ("relu", "gelu", "sigmoid", "softplus", "silu")
TAIL_HW = (3, 5)   # the two low-resolution depth maps of conv2d_tail


def R(id_, entry, n, h, w, cin, cout, kern, **o):
    assert set(o) <= set(DEFAULTS), o
    if entry == "pre":
        o = dict(o, pre=True)
    return Row(id_, entry, n, h, w, cin, cout, kern, tuple(sorted(o.items())))


def opts(row):
    return dict(DEFAULTS, **dict(row.o))


F_OF = {32: "F32", 64: "F64", 128: "F128"}
H_OF = {32: "H32", 64: "H64", 128: "H128"}
WIDTH_COUT = ((32, 32), (64, 64), (128, 130))   # tile width -> the geometry rows' cout (130: tiles_n = 2, the second N-tile 2 channels wide)

# geometry: (n, h, w, the width has a remainder strip).  main tiles (tiles_n = 1): 1, 3, 1, 4, 2, 4, 10, 9, 12, 7, 8, 9, 30
GEOM_SHAPES = [
    (1, 4, 24, False),    # the contract's lower edge: a half-empty tile
    (3, 5, 25, False),
    (1, 8, 32, False),    # the exact tile
    (1, 9, 33, False),    # 2 x 2 tiles, one live row / column in the second ones; no strip (w < 64)
    (1, 8, 65, True),     # strip with one live column
    (1, 9, 72, True),     # a full 8-column strip
    (1, 33, 66, True),    # two 32-row strip tiles, the second with one live row
    (3, 5, 73, False),    # 64 + 9: no strip, a 9-pixel partial tile; 9 main tiles
    (3, 16, 64, False),   # 12 main tiles: q = 1, r = 4 in decode
    (1, 50, 24, False),   # 7 main tiles
    (1, 64, 24, False),   # 8
    (1, 65, 24, False),   # 9
    (3, 33, 66, True),    # 30 main tiles; strip workgroups 6 (tiles_n = 1) / 12 (tiles_n = 2)
]
GEOMETRY = [R(f"geo-{n}x{h}x{w}-bn{bn}", "conv2d", n, h, w, 32, cout, ("I64" if strip else F_OF[bn], H_OF[bn]))
            for (n, h, w, strip) in GEOM_SHAPES for bn, cout in WIDTH_COUT]

S933 = (1, 9, 33)   # ragged on both axes, no strip
S972 = (1, 9, 72)   # 2 x 2 tiles + one strip tile
CHANNELS_IN = [
    # partial and single slabs: the loader's range check returns zeros beyond roundup(cin, 4); [cin, roundup(cin, 4)) is read
    R("ci4-32", "conv2d", *S933, 4, 32, ("F32", "H32")),
    R("ci6-32", "conv2d", *S933, 6, 32, ("F32", "H32")),
    R("ci20-32", "conv2d", *S933, 20, 32, ("F32", "H32")),
    R("ci32-32", "conv2d", *S933, 32, 32, ("F32", "H32")),
    R("ci36-32", "conv2d", *S933, 36, 32, ("F32", "H32")),
    R("ci6-64", "conv2d", *S933, 6, 64, ("F64", "H64")),
    R("ci36-64", "conv2d", *S933, 36, 64, ("F64", "H64")),
    R("ci20-130", "conv2d", *S933, 20, 130, ("F128", "H128")),
    # the tail step (cin > 32, cin % 32 == 2) on the double-buffered 128-column kernel: cchunks 1, 2, 3, 4 -> halo buffer 1, 0, 1, 0;
    # on a strip shape, so that the 32 x 8 tiles take it too
    R("ci34-130", "conv2d", *S972, 34, 130, ("I64", "H128")),
    R("ci66-130", "conv2d", *S972, 66, 130, ("I64", "H128")),
    R("ci98-130", "conv2d", *S972, 98, 130, ("I64", "H128")),
    R("ci130-130", "conv2d", *S972, 130, 130, ("I64", "H128")),
    R("ci66-128-933", "conv2d", *S933, 66, 128, ("F128", "H128")),
    R("ci98-128-933", "conv2d", *S933, 98, 128, ("F128", "H128")),
    # ... and on each narrow kernel (one halo buffer)
    R("ci34-32", "conv2d", *S972, 34, 32, ("I64", "H32")),
    R("ci66-32", "conv2d", *S972, 66, 32, ("I64", "H32")),
    R("ci34-64", "conv2d", *S972, 34, 64, ("I64", "H64")),
    R("ci66-64", "conv2d", *S972, 66, 64, ("I64", "H64")),
    R("ci258-32", "conv2d", *S933, 258, 32, ("F32", "H32")),
    # input ReLU: the tail step reads the staged slab, so the ReLU must already be in it
    R("ci66-130-relu", "conv2d", *S972, 66, 130, ("I64", "H128"), relu_in=True),
    R("ci34-32-relu", "conv2d", *S933, 34, 32, ("F32", "H32"), relu_in=True),
    R("ci32-64-relu", "conv2d", *S933, 32, 64, ("F64", "H64"), relu_in=True),
    # sources that are channel slices
    R("ci32-32-xs", "conv2d", *S933, 32, 32, ("F32", "H32"), xs=(8, 48)),
    R("ci20-64-xs", "conv2d", *S933, 20, 64, ("F64", "H64"), xs=(4, 32)),
    R("ci6-32-xs", "conv2d", *S933, 6, 32, ("F32", "H32"), xs=(4, 16)),
    R("ci34-64-xs", "conv2d", *S972, 34, 64, ("I64", "H64"), xs=(4, 48)),
    R("ci66-130-xs", "conv2d", *S972, 66, 130, ("I64", "H128"), xs=(8, 80)),
]

CHANNELS_OUT = (
    [R(f"co{c}", "conv2d", *S933, 32, c, (F_OF[bn], H_OF[bn])) for c, bn in
     ((8, 32), (20, 32), (32, 32), (33, 64), (40, 64), (64, 64), (66, 128), (98, 128), (128, 128), (130, 128), (194, 128))] +
    # 98 dense above: ldy = 100, the 16-byte path writes channels 98, 99 as zeros; here in a wide slice: the scalar path writes exactly 98
    [R("co98-slice", "conv2d", *S933, 32, 98, ("F128", "H128"), ys=(4, 108)),
     R("co33-slice-c0-2", "conv2d", *S933, 32, 33, ("F64", "H64"), ys=(2, 40)),        # first channel no multiple of 4
     R("co64-slice", "conv2d", *S933, 32, 64, ("F64", "H64"), ys=(8, 80)),             # 16-byte path with ldy > cout
     R("co256-gamma", "conv2d", *S933, 32, 256, ("F128", "H128"), gamma=True),         # gamma leaves the c256 rung: halo16<128>, tiles_n = 2
     # ragged channels in the 32 x 8 strip tiles
     R("co98-strip", "conv2d", *S972, 32, 98, ("I64", "H128")),
     R("co130-strip", "conv2d", *S972, 32, 130, ("I64", "H128")),
     R("co194-strip", "conv2d", *S972, 32, 194, ("I64", "H128")),
     R("co33-strip", "conv2d", *S972, 32, 33, ("I64", "H64")),
     R("co66-mul-wide", "conv2d", *S933, 32, 66, ("F128", "H128"), mul=True, wide=True)])   # scalar path with a strided operand

EPI_WIDTHS = ((32, 32), (64, 64), (128, 128))   # tile width -> cout (a fused LayerNorm needs cout <= 128)
EPILOGUE = []
for _bn, _c in EPI_WIDTHS:
    _k = (F_OF[_bn], H_OF[_bn])
    EPILOGUE += [
        # lean store loops (bf16 modes): bias + act, bias + LN + act, bias + act + res -- all five activations on the first
        *[R(f"ep{_bn}-{a}", "conv2d", *S933, 32, _c, _k, act=a) for a in ACTS],
        R(f"ep{_bn}-ln-relu", "conv2d", *S933, 32, _c, _k, ln=True, act="relu"),
        R(f"ep{_bn}-ln-gelu", "conv2d", *S933, 32, _c, _k, ln=True, act="gelu"),
        R(f"ep{_bn}-relu-res", "conv2d", *S933, 32, _c, _k, act="relu", res=True),
        R(f"ep{_bn}-res-wide", "conv2d", 3, 9, 33, 32, _c, _k, res=True, wide=True),
        R(f"ep{_bn}-nobias-relu", "conv2d", *S933, 32, _c, _k, bias=False, act="relu"),
        # the general epi_store loop (erf GELU)
        R(f"ep{_bn}-gamma-gelu", "conv2d", *S933, 32, _c, _k, gamma=True, act="gelu"),
        R(f"ep{_bn}-mul", "conv2d", *S933, 32, _c, _k, mul=True),
        R(f"ep{_bn}-res2", "conv2d", *S933, 32, _c, _k, res2=True, act="sigmoid"),
        R(f"ep{_bn}-ln-res", "conv2d", *S933, 32, _c, _k, ln=True, res=True, act="softplus"),
        R(f"ep{_bn}-all", "conv2d", 3, 9, 33, 32, _c, _k, ln=True, act="silu", gamma=True, mul=True, res=True, res2=True, wide=True),
        R(f"ep{_bn}-all-nobias", "conv2d", *S933, 32, _c, _k, bias=False, act="relu", gamma=True, mul=True, res=True, res2=True),
        # a common offset of 40 in front of the LayerNorm: one-pass statistics would miss the bar
        R(f"ep{_bn}-ln-offset", "conv2d", *S933, 32, _c, _k, ln=True, act="relu", bias_offset=40.0),
    ]
EPILOGUE += [
    R("ep-ln-co20", "conv2d", *S933, 32, 20, ("F32", "H32"), ln=True, act="gelu"),          # ln_row_stats' scalar remainder: b + 8 > Cout
    R("ep-ln-co40-res", "conv2d", *S933, 32, 40, ("F64", "H64"), ln=True, res=True),
    R("ep-ln-co98", "conv2d", *S933, 32, 98, ("F128", "H128"), ln=True, act="relu"),        # LN over a ragged row, pad channels zero
    R("ep-ln-strip-128", "conv2d", *S972, 32, 128, ("I128", "H128"), ln=True, act="relu"),  # f32 strip with LN: the 128-column generic kernel
    R("ep-all-strip-64", "conv2d", *S972, 66, 64, ("I64", "H64"), ln=True, act="gelu", gamma=True, mul=True, res=True, res2=True, wide=True),
]

CONV_ROWS = GEOMETRY + CHANNELS_IN + CHANNELS_OUT + EPILOGUE

PRE_ROWS = [
    R("pre-32", "pre", *S933, 32, 32, (None, "H32")),
    R("pre-64-gelu", "pre", *S933, 32, 64, (None, "H64"), act="gelu"),
    R("pre-128", "pre", *S933, 32, 128, (None, "H128")),
    R("pre-132", "pre", *S933, 32, 132, (None, "H128")),                      # the second N-tile carries 4 channels of the addend
    R("pre-ln-32", "pre", *S933, 32, 32, (None, "H32"), ln=True, act="relu"),
    R("pre-ln-64", "pre", 3, 9, 33, 32, 64, (None, "H64"), ln=True, act="relu", wide=True),
    R("pre-ln-128", "pre", *S933, 32, 128, (None, "H128"), ln=True),
    R("pre-res-32", "pre", *S933, 32, 32, (None, "H32"), res=True, act="relu"),
    R("pre-res-128", "pre", 3, 9, 33, 32, 128, (None, "H128"), res=True, wide=True),
    R("pre-strip-32", "pre", *S972, 32, 32, (None, "H32")),
    R("pre-strip-64", "pre", 1, 33, 66, 32, 64, (None, "H64"), ln=True),
    R("pre-strip-128", "pre", *S972, 32, 128, (None, "H128"), wide=True),
    R("pre-tailstep-32", "pre", *S933, 66, 32, (None, "H32")),
    R("pre-tailstep-64", "pre", *S972, 34, 64, (None, "H64")),
    R("pre-tailstep-128", "pre", *S972, 98, 128, (None, "H128"), ln=True, act="relu"),
]

TAIL_ROWS = [
    R("tail-8", "tail", *S933, 32, 8, (None, "H32")),
    R("tail-32", "tail", *S933, 32, 32, (None, "H32")),
    R("tail-64-relu", "tail", *S933, 32, 64, (None, "H64"), act="relu"),
    R("tail-128", "tail", *S933, 32, 128, (None, "H128")),                    # the widest the entry point takes (tiles_n = 1)
    R("tail-ln-32", "tail", 3, 9, 33, 32, 32, (None, "H32"), ln=True, act="relu"),
    R("tail-ln-64", "tail", *S933, 32, 64, (None, "H64"), ln=True),
    R("tail-ln-128", "tail", *S933, 32, 128, (None, "H128"), ln=True, act="gelu"),
    R("tail-strip-32", "tail", *S972, 32, 32, (None, "H32")),
    R("tail-strip-64", "tail", 1, 33, 66, 32, 64, (None, "H64")),
    R("tail-strip-128", "tail", *S972, 32, 128, (None, "H128"), ln=True, act="relu"),
    R("tail-c0-4", "tail", *S933, 32, 32, (None, "H32"), ys=(4, 40)),         # the filled row starts behind other channels
    R("tail-tailstep-64", "tail", *S972, 66, 64, (None, "H64")),
]

CONV_CASES = [(r, m) for r in CONV_ROWS for m in MODES3]
PRE_CASES = [(r, m) for r in PRE_ROWS for m in MODES2]
TAIL_CASES = [(r, m) for r in TAIL_ROWS for m in MODES2]
ALL_ROWS = CONV_ROWS + PRE_ROWS + TAIL_ROWS
ROW_BY_ID = {r.id: r for r in ALL_ROWS}

# consistency: a second call is bit-equal; image 1 of a batch of 3 is bit-equal to the same image alone; halo == force_generic at 2e-5
REPEAT_IDS = ["geo-3x33x66-bn128", "ci66-130", "ci34-32", "ep64-all", "pre-ln-64", "tail-ln-32"]
BATCH_IDS = ["geo-3x5x25-bn32", "geo-3x16x64-bn64", "geo-3x33x66-bn128", "ep32-all", "ep128-res-wide", "pre-res-128", "tail-ln-32"]
GENERIC_IDS = ["geo-1x9x33-bn32", "geo-1x9x72-bn64", "geo-3x33x66-bn128", "ci66-130", "ci34-64", "co98", "ep64-all", "ep128-gamma-gelu"]
GENERIC_TOL = 2e-5


def row_id(v):
    return v.id if isinstance(v, Row) else str(v)


def expected_kernel(row, mode):
    key = row.kern[0] if mode == "f32" else row.kern[1]
    return KERNEL[key].format(mode)


def bf16_bar(emu):
    return min(4.0 * emu, BF16_CAP)


# ---- layout rules the buffers follow ------------------------------------------------------------------------------------------------------

def dst_layout(row):
    """(first channel, pixel stride) of the destination"""
    o = opts(row)
    extra = 4 if row.entry == "tail" else 0
    if o["ys"] is not None:
        return o["ys"]
    return 0, roundup(row.cout, 4) + extra


def operand_layout(row):
    """(first channel, pixel stride) of mul / res / res2 / pre"""
    c4 = roundup(row.cout, 4)
    return (4, c4 + 8) if opts(row)["wide"] else (0, c4)


def vec_epi(row):
    """conv_fill_params' 16-byte epilogue rule: every pointer 16-byte aligned, every pixel stride a multiple of 4, and -- cout % 4 != 0 --
    nothing but the pad channels behind cout (which the op then owns and writes as zeros)"""
    o = opts(row)
    c4, padded = roundup(row.cout, 4), row.cout % 4 != 0
    lays = [dst_layout(row)] + [operand_layout(row) for k in ("mul", "res", "res2") if o[k]]
    return all(ld % 4 == 0 and c0 % 4 == 0 and (not padded or ld == c4) for c0, ld in lays)


# ---- data, float64 reference, bf16 emulation -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inputs(row):
    """CPU fp32 operands of a row (NCHW), made once and never written again"""
    o = opts(row)
    n, h, w, cin, cout = row.n, row.h, row.w, row.cin, row.cout
    sd = zlib.crc32(row.id.encode()) % (2 ** 30)
    ph, pw = TAIL_HW
    return dict(x=rnd(sd + 1, n, cin, h, w), w=rnd(sd + 2, cout, cin, 3, 3) / math.sqrt(9 * cin), b=0.5 * rnd(sd + 3, cout) + o["bias_offset"],
                lnw=1 + 0.2 * rnd(sd + 4, cout), lnb=0.1 * rnd(sd + 5, cout), gamma=1 + 0.3 * rnd(sd + 6, cout), mul=rnd(sd + 7, n, cout, h, w),
                res=rnd(sd + 8, n, cout, h, w), res2=rnd(sd + 9, n, cout, h, w), pre=0.5 * rnd(sd + 10, n, cout, h, w),
                p1=rnd(sd + 11, n, 1, ph, pw).abs(), p2=rnd(sd + 12, n, 1, ph, pw).abs())


def ln_two_pass(y, lnw, lnb, eps=1e-6):
    u = y.mean(1, keepdim=True)
    var = (y - u).pow(2).mean(1, keepdim=True)
    return (y - u) / torch.sqrt(var + eps) * lnw.view(1, -1, 1, 1) + lnb.view(1, -1, 1, 1)


def activation(t, act, gelu="erf"):
    if act == "relu":
        return F.relu(t)
    if act == "gelu":
        return F.gelu(t) if gelu == "erf" else F.gelu(t, approximate="tanh")
    if act == "sigmoid":
        return torch.sigmoid(t)
    if act == "softplus":
        return F.softplus(t, beta=1.0, threshold=20.0)
    if act == "silu":
        return F.silu(t)
    assert act == "none"
    return t


def bf16r(t):
    return t.float().to(torch.bfloat16).to(t.dtype)


def evaluate(row, dt=torch.float64, bf16=False, drop=(), gelu="erf", ln=ln_two_pass, x=None):
    """the row's graph in plain torch, in ``dt``.  bf16: x (behind the input ReLU) and the weights rounded to bf16 first; drop: switches of the
    row to leave out; x: another input in place of the row's"""
    d = inputs(row)
    o = dict(opts(row), **{k: (False if k != "act" else "none") for k in drop})
    c = lambda t: t.to(dt)  # noqa: E731
    ch = lambda t: c(t).view(1, -1, 1, 1)  # noqa: E731
    xv, wv = c(d["x"] if x is None else x), c(d["w"])
    if o["relu_in"]:
        xv = F.relu(xv)
    if bf16:
        xv, wv = bf16r(xv), bf16r(wv)
    y = F.conv2d(xv, wv, None, padding=1)
    if o["bias"]:
        y = y + ch(d["b"])
    if o["pre"]:
        y = y + c(d["pre"])
    if o["ln"]:
        y = ln(y, c(d["lnw"]), c(d["lnb"]))
    y = activation(y, o["act"], gelu)
    if o["gamma"]:
        y = y * ch(d["gamma"])
    if o["mul"]:
        y = y * c(d["mul"])
    if o["res"]:
        y = y + c(d["res"])
    if o["res2"]:
        y = y + c(d["res2"])
    if row.entry == "tail":
        pair = [F.interpolate(c(d[k]), (row.h, row.w), mode="bilinear", align_corners=True) for k in ("p1", "p2")]
        y = torch.cat([y] + pair + [torch.zeros(row.n, 2, row.h, row.w, dtype=dt)], 1)
    return y


@functools.lru_cache(maxsize=None)
def reference(row):
    return evaluate(row)


@functools.lru_cache(maxsize=None)
def emulation(row):
    return evaluate(row, bf16=True)


def emulation_error(row):
    ref = reference(row)
    return float((emulation(row) - ref).abs().max()) / max(1.0, float(ref.abs().max()))


# error of ``emulation`` against ``reference`` as a share of max(1, |ref|max), measured on the CPU (tests/test_halo_conv_host.py recomputes it)
EMU = {
    "geo-1x4x24-bn32": 2.195e-03, "geo-1x4x24-bn64": 2.317e-03, "geo-1x4x24-bn128": 2.522e-03, "geo-3x5x25-bn32": 2.250e-03,
    "geo-3x5x25-bn64": 2.210e-03, "geo-3x5x25-bn128": 2.221e-03, "geo-1x8x32-bn32": 2.166e-03, "geo-1x8x32-bn64": 2.352e-03,
    "geo-1x8x32-bn128": 2.137e-03, "geo-1x9x33-bn32": 2.206e-03, "geo-1x9x33-bn64": 1.970e-03, "geo-1x9x33-bn128": 2.081e-03,
    "geo-1x8x65-bn32": 2.282e-03, "geo-1x8x65-bn64": 2.202e-03, "geo-1x8x65-bn128": 2.223e-03, "geo-1x9x72-bn32": 2.809e-03,
    "geo-1x9x72-bn64": 2.275e-03, "geo-1x9x72-bn128": 2.045e-03, "geo-1x33x66-bn32": 1.985e-03, "geo-1x33x66-bn64": 2.194e-03,
    "geo-1x33x66-bn128": 2.068e-03, "geo-3x5x73-bn32": 2.148e-03, "geo-3x5x73-bn64": 2.464e-03, "geo-3x5x73-bn128": 2.181e-03,
    "geo-3x16x64-bn32": 1.848e-03, "geo-3x16x64-bn64": 2.203e-03, "geo-3x16x64-bn128": 1.928e-03, "geo-1x50x24-bn32": 2.162e-03,
    "geo-1x50x24-bn64": 2.071e-03, "geo-1x50x24-bn128": 2.521e-03, "geo-1x64x24-bn32": 2.098e-03, "geo-1x64x24-bn64": 2.395e-03,
    "geo-1x64x24-bn128": 2.142e-03, "geo-1x65x24-bn32": 1.998e-03, "geo-1x65x24-bn64": 1.985e-03, "geo-1x65x24-bn128": 2.482e-03,
    "geo-3x33x66-bn32": 2.317e-03, "geo-3x33x66-bn64": 2.454e-03, "geo-3x33x66-bn128": 2.074e-03, "ci4-32": 2.091e-03, "ci6-32": 2.881e-03,
    "ci20-32": 2.254e-03, "ci32-32": 1.978e-03, "ci36-32": 2.229e-03, "ci6-64": 2.504e-03, "ci36-64": 2.065e-03, "ci20-130": 2.333e-03,
    "ci34-130": 1.864e-03, "ci66-130": 1.979e-03, "ci98-130": 1.950e-03, "ci130-130": 2.302e-03, "ci66-128-933": 2.383e-03, "ci98-128-933": 2.066e-03,
    "ci34-32": 2.025e-03, "ci66-32": 2.261e-03, "ci34-64": 2.573e-03, "ci66-64": 2.270e-03, "ci258-32": 2.281e-03, "ci66-130-relu": 2.223e-03,
    "ci34-32-relu": 2.710e-03, "ci32-64-relu": 1.965e-03, "ci32-32-xs": 2.145e-03, "ci20-64-xs": 2.190e-03, "ci6-32-xs": 2.852e-03,
    "ci34-64-xs": 1.895e-03, "ci66-130-xs": 2.214e-03, "co8": 2.307e-03, "co20": 1.577e-03, "co32": 1.726e-03, "co33": 2.050e-03, "co40": 2.453e-03,
    "co64": 2.276e-03, "co66": 2.119e-03, "co98": 1.873e-03, "co128": 2.084e-03, "co130": 2.113e-03, "co194": 2.127e-03, "co98-slice": 2.762e-03,
    "co33-slice-c0-2": 1.696e-03, "co64-slice": 1.714e-03, "co256-gamma": 2.178e-03, "co98-strip": 2.279e-03, "co130-strip": 2.372e-03,
    "co194-strip": 1.945e-03, "co33-strip": 2.153e-03, "co66-mul-wide": 2.727e-03, "ep32-relu": 2.032e-03, "ep32-gelu": 1.828e-03,
    "ep32-sigmoid": 2.523e-03, "ep32-softplus": 1.584e-03, "ep32-silu": 2.892e-03, "ep32-ln-relu": 2.721e-03, "ep32-ln-gelu": 3.069e-03,
    "ep32-relu-res": 1.719e-03, "ep32-res-wide": 2.007e-03, "ep32-nobias-relu": 2.516e-03, "ep32-gamma-gelu": 2.825e-03, "ep32-mul": 1.527e-03,
    "ep32-res2": 5.420e-04, "ep32-ln-res": 1.288e-03, "ep32-all": 2.004e-03, "ep32-all-nobias": 1.862e-03, "ep32-ln-offset": 2.641e-03,
    "ep64-relu": 2.391e-03, "ep64-gelu": 2.360e-03, "ep64-sigmoid": 2.521e-03, "ep64-softplus": 1.517e-03, "ep64-silu": 1.766e-03,
    "ep64-ln-relu": 2.577e-03, "ep64-ln-gelu": 2.779e-03, "ep64-relu-res": 1.766e-03, "ep64-res-wide": 1.645e-03, "ep64-nobias-relu": 2.864e-03,
    "ep64-gamma-gelu": 1.862e-03, "ep64-mul": 2.053e-03, "ep64-res2": 4.729e-04, "ep64-ln-res": 1.477e-03, "ep64-all": 2.660e-03,
    "ep64-all-nobias": 2.244e-03, "ep64-ln-offset": 2.254e-03, "ep128-relu": 2.170e-03, "ep128-gelu": 2.065e-03, "ep128-sigmoid": 2.373e-03,
    "ep128-softplus": 2.018e-03, "ep128-silu": 2.420e-03, "ep128-ln-relu": 2.214e-03, "ep128-ln-gelu": 2.114e-03, "ep128-relu-res": 1.410e-03,
    "ep128-res-wide": 1.445e-03, "ep128-nobias-relu": 2.290e-03, "ep128-gamma-gelu": 2.317e-03, "ep128-mul": 2.249e-03, "ep128-res2": 5.150e-04,
    "ep128-ln-res": 1.161e-03, "ep128-all": 2.261e-03, "ep128-all-nobias": 1.939e-03, "ep128-ln-offset": 2.266e-03, "ep-ln-co20": 3.498e-03,
    "ep-ln-co40-res": 1.706e-03, "ep-ln-co98": 2.133e-03, "ep-ln-strip-128": 2.301e-03, "ep-all-strip-64": 2.649e-03, "pre-32": 2.189e-03,
    "pre-64-gelu": 2.279e-03, "pre-128": 1.721e-03, "pre-132": 2.067e-03, "pre-ln-32": 2.098e-03, "pre-ln-64": 2.891e-03, "pre-ln-128": 1.789e-03,
    "pre-res-32": 1.418e-03, "pre-res-128": 1.662e-03, "pre-strip-32": 1.590e-03, "pre-strip-64": 2.251e-03, "pre-strip-128": 1.978e-03,
    "pre-tailstep-32": 1.738e-03, "pre-tailstep-64": 2.052e-03, "pre-tailstep-128": 1.671e-03, "tail-8": 1.994e-03, "tail-32": 1.759e-03,
    "tail-64-relu": 1.589e-03, "tail-128": 2.509e-03, "tail-ln-32": 3.315e-03, "tail-ln-64": 1.987e-03, "tail-ln-128": 2.243e-03,
    "tail-strip-32": 2.276e-03, "tail-strip-64": 2.018e-03, "tail-strip-128": 1.767e-03, "tail-c0-4": 2.337e-03, "tail-tailstep-64": 1.982e-03,
}


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------------

def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def source(P, t, sl):
    """the conv's input: channels [c0, c0 + cin) of a NaN buffer; the loader's pad channels [cin, roundup(cin, 4)) behind them hold BIG"""
    v = nhwc(t)
    c = v.shape[3]
    c0, ld = sl if sl is not None else (0, roundup(c, 4))
    buf = torch.full((*v.shape[:3], ld), NAN)
    buf[..., c0:c0 + c] = v
    buf[..., c0 + c:c0 + roundup(c, 4)] = BIG
    return P.Feat(buf.to(DEV), c, c0)


def operand(P, t, lay):
    """mul / res / res2 / pre: channels [c0, c0 + cout) of a buffer that is NaN everywhere else (pad channels included)"""
    v = nhwc(t)
    c0, ld = lay
    buf = torch.full((*v.shape[:3], ld), NAN)
    buf[..., c0:c0 + v.shape[3]] = v
    return P.Feat(buf.to(DEV), v.shape[3], c0)


def destination(P, row, n):
    """NaN where the op must write -- its channels, the four of the depth pair, the pad channels the 16-byte path owns -- SENTINEL elsewhere.
    -> (Feat, number of channels written behind the first, number of those that must come back zero)"""
    c0, ld = dst_layout(row)
    nwrite = row.cout + (4 if row.entry == "tail" else 0)
    nzero = 0
    if row.cout % 4 and vec_epi(row):
        nzero = roundup(row.cout, 4) - row.cout
    buf = torch.full((n, row.h, row.w, ld), SENTINEL)
    buf[..., c0:c0 + nwrite + nzero] = NAN
    return P.Feat(buf.to(DEV), row.cout, c0), nwrite, nzero


def run_row(P, row, mode, img=None, force_generic=False):
    """-> (NCHW result on the CPU, kernel name).  img: run this image of the batch alone"""
    o, d = opts(row), inputs(row)
    pick = (lambda t: t) if img is None else (lambda t: t[img:img + 1])
    n = row.n if img is None else 1
    dev = lambda t: t.to(DEV)  # noqa: E731
    cw = P.pack_conv(dev(d["w"]), dev(d["b"]) if o["bias"] else None, pad=1, prec=P.L.PREC_NAMES[mode])
    x = source(P, pick(d["x"]), o["xs"])
    aux = {k: operand(P, pick(d[k]), operand_layout(row)) for k in ("mul", "res", "res2", "pre") if o[k]}
    dst, nwrite, nzero = destination(P, row, n)
    ln = (dev(d["lnw"]), dev(d["lnb"])) if o["ln"] else None
    act = getattr(P.L, "ACT_" + o["act"].upper())
    if row.entry == "conv2d":
        P.conv2d(x, cw, dst, relu_in=o["relu_in"], act=act, gamma=dev(d["gamma"]) if o["gamma"] else None, mul=aux.get("mul"), res=aux.get("res"),
                 res2=aux.get("res2"), ln=ln, force_generic=force_generic)
    elif row.entry == "pre":
        assert P.conv2d_pre_supported(row.h, row.w, cw, ln is not None)
        P.conv2d_pre(x, cw, aux["pre"], dst, act=act, res=aux.get("res"), ln=ln)
    else:
        assert P.conv2d_tail_supported(x, cw, dst)
        P.conv2d_tail(x, cw, dst, P.Feat(dev(nhwc(pick(d["p1"])))), P.Feat(dev(nhwc(pick(d["p2"])))), act=act, ln=ln)
    name = last_kernel(P)
    buf = dst.buf.cpu()
    c0 = dst.c0
    # every channel the op does not own comes back untouched; the pad channels it owns come back zero
    assert bool((buf[..., :c0] == SENTINEL).all()) and bool((buf[..., c0 + nwrite + nzero:] == SENTINEL).all()), f"{row.id} {mode}: wrote outside its channels"
    assert bool((buf[..., c0 + nwrite:c0 + nwrite + nzero] == 0).all()), f"{row.id} {mode}: pad channels of the 16-byte path are not zero"
    return buf[..., c0:c0 + nwrite].permute(0, 3, 1, 2).contiguous(), name


def check_row(P, row, mode):
    got, name = run_row(P, row, mode)
    assert name == expected_kernel(row, mode), (row.id, mode, name, expected_kernel(row, mode))
    what = f"{row.entry} {row.id} {mode}"
    if mode == "bf16":
        bar = bf16_bar(EMU[row.id])
        assert 0 < bar <= BF16_CAP
        close(got, reference(row), bar, what)
        close(got, emulation(row), BF16_EMU_TOL, what + " vs emulation")
    else:
        close(got, reference(row), TOL[mode], what)


@pytest.mark.parametrize("row,mode", CONV_CASES, ids=[f"{r.id}-{m}" for r, m in CONV_CASES])
def test_conv2d_rows(P, row, mode):
    check_row(P, row, mode)


@pytest.mark.parametrize("row,mode", PRE_CASES, ids=[f"{r.id}-{m}" for r, m in PRE_CASES])
def test_conv2d_pre_rows(P, row, mode):
    check_row(P, row, mode)


@pytest.mark.parametrize("row,mode", TAIL_CASES, ids=[f"{r.id}-{m}" for r, m in TAIL_CASES])
def test_conv2d_tail_rows(P, row, mode):
    check_row(P, row, mode)


def test_conv2d_tail_refuses_more_than_128_channels(P):
    """cout 130 would give the depth pair to the last of two N-tiles, but the entry point's contract stops at cout % 4 == 0 and cout <= 128
    (tail_shape_ok): it says so instead of running"""
    for cout in (130, 132):
        row = R(f"tail-{cout}-refused", "tail", *S933, 32, cout, (None, "H128"), ys=(2, 136) if cout == 130 else None)
        d = inputs(row)
        cw = P.pack_conv(d["w"].to(DEV), d["b"].to(DEV), pad=1, prec=P.L.PREC_NAMES["bf16x3"])
        x = source(P, d["x"], None)
        dst, _, _ = destination(P, row, row.n)
        assert dst.ld == dst.c0 + cout + 4 and (dst.c0 + cout) % 4 == 0
        assert not P.conv2d_tail_supported(x, cw, dst)
        with pytest.raises(RuntimeError):
            P.conv2d_tail(x, cw, dst, P.Feat(nhwc(d["p1"]).to(DEV)), P.Feat(nhwc(d["p2"]).to(DEV)))
        assert bool((dst.buf.cpu()[..., :dst.c0] == SENTINEL).all())


def modes_of(row):
    return MODES3 if row.entry == "conv2d" else MODES2


@pytest.mark.parametrize("rid", REPEAT_IDS)
def test_second_call_is_bit_equal(P, rid):
    row = ROW_BY_ID[rid]
    for mode in modes_of(row):
        a, b = run_row(P, row, mode)[0], run_row(P, row, mode)[0]
        assert torch.equal(a, b), (rid, mode, int((a != b).sum()))


@pytest.mark.parametrize("rid", BATCH_IDS)
def test_image_of_a_batch_is_bit_equal_to_the_image_alone(P, rid):
    row = ROW_BY_ID[rid]
    assert row.n == 3
    for mode in modes_of(row):
        (batch, k3), (alone, k1) = run_row(P, row, mode), run_row(P, row, mode, img=1)
        assert k3 == k1 == expected_kernel(row, mode)
        assert torch.equal(batch[1:2], alone), (rid, mode, int((batch[1:2] != alone).sum()), float((batch[1:2] - alone).abs().max()))


@pytest.mark.parametrize("rid", GENERIC_IDS)
def test_halo_agrees_with_the_generic_kernel(P, rid):
    row = ROW_BY_ID[rid]
    for mode in ("f32", "bf16x3"):
        (halo, kh), (gen, kg) = run_row(P, row, mode), run_row(P, row, mode, force_generic=True)
        assert kh == expected_kernel(row, mode) and kg.startswith("igemm_kernel<"), (kh, kg)
        close(halo, gen.double(), GENERIC_TOL, f"{rid} {mode} halo vs generic")
