"""GPU parity of the gather side -- csrc/gather.hip (bilinear align_corners upsample, depth_pair_fill, roi_align, crop_resize, the layout
changes) and the ZoeDepth-head, token and pad kernels of csrc/pointwise.hip -- against plain torch in float64 on the CPU, at the smallest
shapes that still take each launch path.  The references share nothing with the kernels' tap arithmetic: F.interpolate and
F.grid_sample in float64, the formulas of oracle/zoe.py in float64, reshapes.  The tables and the reference side need no GPU and no
library: tests/test_resample_kernels_host.py checks them (launch path of every row against a restatement of the launchers' predicates,
the float32 oracle's share of every tolerance, discrimination, the ROI discontinuity margins).

Inputs go into ``Feat`` buffers and results come out of ``feat.buf`` with plain torch indexing -- never through Feat.from_nchw / to_nchw, so
the layout kernels (group e) can neither mask nor cause a failure of another group.  A destination the test hands to an op is NaN where
the op must write and holds a sentinel in every other channel.  (zoe_*, patchify and assemble_tokens allocate their own result.)
Every comparison prints ``err / tol`` before it asserts."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import zoe as o_zoe  # noqa: E402

DEV = "cuda"
NAN = float("nan")
SENT = -7.5                 # what every channel beside a destination slice holds before and after
EPS = 2.0 ** -23


@pytest.fixture(scope="module")
def P():
    from patchrefinerv2_amd import ops
    ops.L.load()
    return ops


def rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def roundup(a, b):
    return (a + b - 1) // b * b


def dense_ld(c):
    """the pixel stride of an un-sliced map: one channel is stored dense (Feat.alloc(pad_to=1)), everything else padded to 4"""
    return 1 if c == 1 else roundup(c, 4)


def within(got, ref, tol, what):
    """absolute: max|got - ref| <= tol, the output finite; prints the share of the tolerance used"""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = float((got - ref.double()).abs().max())
    print(f"[resample] {what}: err {err:.3e} tol {tol:.3e} ratio {err / tol if tol else 0.0:.3f}")
    assert err <= tol, f"{what}: max|d| = {err:.3e} > {tol:.3e}"


def src_feat(P, x, c0, ld):
    """x [n, c, h, w] as the channels [c0, c0 + c) of a fresh ld-channel NHWC buffer that is NaN elsewhere"""
    n, c, h, w = x.shape
    buf = torch.full((n, h, w, ld), NAN)
    buf[..., c0:c0 + c] = x.permute(0, 2, 3, 1)
    return P.Feat(buf.to(DEV)).slice(c0, c)


def dst_feat(P, n, h, w, c, c0, ld):
    """a destination: NaN in the channels [c0, c0 + c), SENT in every other one"""
    buf = torch.full((n, h, w, ld), SENT)
    buf[..., c0:c0 + c] = NAN
    return P.Feat(buf.to(DEV)).slice(c0, c)


def read(feat):
    """-> the destination slice as [n, c, h, w] on the CPU; asserts that its neighbours still hold SENT"""
    got = feat.buf.cpu()
    rest = torch.cat([got[..., :feat.c0], got[..., feat.c0 + feat.c:]], -1)
    assert bool((rest == SENT).all()), "channels beside the destination slice were written"
    return got[..., feat.c0:feat.c0 + feat.c].permute(0, 3, 1, 2).contiguous()


def neighbour_diffs(x):
    """(Dy, Dx, max|x|) of x [..., h, w]: the largest differences of vertically / horizontally adjacent values"""
    dy = float((x[..., 1:, :] - x[..., :-1, :]).abs().max()) if x.shape[-2] > 1 else 0.0
    dx = float((x[..., :, 1:] - x[..., :, :-1]).abs().max()) if x.shape[-1] > 1 else 0.0
    return dy, dx, float(x.abs().max())


# ---- a. bilinear, align_corners=True: upsample_bilinear, depth_pair_fill ---------------------------------------------------------------
# (n, c, h, w, oh, ow, launch path).  prv2_upsample_bilinear: vec = c % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 (16-byte aligned);
# "rows" = upsample_bilinear_rows_kernel<4> (vec, oh >= 16), "pixel4" = upsample_bilinear_kernel<4> (vec), "scalar" = ..._kernel<1>
UP_CASES = [
    (2, 8, 6, 9, 17, 23, "rows"),       # oh % 4 == 1: the last block of rows stops after one row
    (1, 4, 7, 5, 18, 11, "rows"),       # oh % 4 == 2
    (1, 12, 9, 8, 19, 30, "rows"),      # oh % 4 == 3
    (1, 8, 40, 31, 16, 11, "rows"),     # down-sampling: source rows jump, the two-entry row cache misses
    (1, 4, 1, 9, 16, 20, "rows"),       # source height 1
    (1, 4, 9, 1, 16, 3, "rows"),        # source width 1
    (1, 8, 16, 12, 16, 12, "rows"),     # identity: the input, bit for bit
    (1, 8, 5, 7, 15, 22, "pixel4"),
    (1, 4, 5, 5, 1, 1, "pixel4"),       # output sizes of 1: ac_scale == 0
    (1, 4, 13, 9, 1, 17, "pixel4"),
    (2, 8, 6, 9, 15, 1, "pixel4"),
    (1, 3, 6, 9, 17, 23, "scalar"),
    (1, 1, 10, 7, 4, 5, "scalar"),
]
# the input is the channels [4, 4 + c) of a (c + 8)-channel buffer, the output the channels [8, 8 + c) of a (c + 12)-channel one
UP_SLICE_CASES = [UP_CASES[0], UP_CASES[7]]
# the same input into a destination of pixel stride c + 1: upsample_bilinear_kernel<1>, whose bits the other two kernels must give
UP_BITEQ_CASES = [UP_CASES[0], UP_CASES[3], UP_CASES[7]]
# depth_pair_fill (n, h, w, oh, ow), at c0 = 0 and c0 = 8
PAIR_CASES = [(2, 6, 9, 17, 23), (1, 40, 31, 16, 11), (1, 5, 5, 1, 1)]
PAIR_C0 = (0, 8)


def up_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}x{c[3]}-to-{c[4]}x{c[5]}"


def up_layout(case, kind):
    """-> (c0x, ldx, c0y, ldy) of a case run "dense", as "slice"s, or into an "odd" destination stride"""
    c = case[1]
    return {"dense": (0, dense_ld(c), 0, dense_ld(c)), "slice": (4, c + 8, 8, c + 12), "odd": (0, dense_ld(c), 0, c + 1)}[kind]


def up_input(case):
    n, c, h, w = case[:4]
    return rnd(100 + UP_CASES.index(case), n, c, h, w)


def bilinear64(x, oh, ow, align_corners=True):
    return F.interpolate(x.double(), (oh, ow), mode="bilinear", align_corners=align_corners)


@functools.lru_cache(maxsize=None)
def up_ref(case):
    return bilinear64(up_input(case), case[4], case[5])


def bilinear_tol(x):
    """eps ((h - 1) Dy + (w - 1) Dx) + 8 eps max|x|, eps = 2^-23.  The source coordinate fl(fl(scale) * dst) is off by at most eps times
    itself (two roundings of 2^-24), so a weight is off by at most eps (h - 1) resp. eps (w - 1), and a weight error multiplies the
    difference of the two neighbours it blends; the last term covers the roundings of 1 - w and of the six multiply-adds"""
    h, w = x.shape[-2:]
    dy, dx, mx = neighbour_diffs(x)
    return EPS * ((h - 1) * dy + (w - 1) * dx) + 8 * EPS * mx


def run_upsample(P, case, kind):
    n, c, h, w, oh, ow, _ = case
    c0x, ldx, c0y, ldy = up_layout(case, kind)
    out = dst_feat(P, n, oh, ow, c, c0y, ldy)
    P.upsample_bilinear(src_feat(P, up_input(case), c0x, ldx), oh, ow, out=out)
    return read(out)


@pytest.mark.parametrize("case", UP_CASES, ids=up_id)
def test_upsample_bilinear(P, case):
    got = run_upsample(P, case, "dense")
    within(got, up_ref(case), bilinear_tol(up_input(case)), f"a upsample {case[6]} {up_id(case)}")
    if case[2:4] == case[4:6]:
        assert torch.equal(got, up_input(case)), "the identity size must copy the input"


@pytest.mark.parametrize("case", UP_SLICE_CASES, ids=up_id)
def test_upsample_bilinear_slice_to_slice(P, case):
    got = run_upsample(P, case, "slice")
    within(got, up_ref(case), bilinear_tol(up_input(case)), f"a upsample slices {case[6]} {up_id(case)}")


@pytest.mark.parametrize("case", UP_BITEQ_CASES, ids=up_id)
def test_upsample_bilinear_kernels_agree_bit_for_bit(P, case):
    """"identical arithmetic per output" (csrc/gather.hip, built with -ffp-contract=off): a row the rows kernel's cache evicted too late, or
    kept for the wrong source row, would differ here"""
    a, b = run_upsample(P, case, "dense"), run_upsample(P, case, "odd")
    within(b, up_ref(case), bilinear_tol(up_input(case)), f"a upsample scalar twin of {up_id(case)}")
    assert torch.equal(a, b)


def pair_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-to-{c[3]}x{c[4]}"


def pair_inputs(case):
    n, h, w = case[:3]
    i = PAIR_CASES.index(case)
    return rnd(120 + i, n, 1, h, w), rnd(130 + i, n, 1, h, w)


@functools.lru_cache(maxsize=None)
def pair_ref(case):
    return tuple(bilinear64(p, case[3], case[4]) for p in pair_inputs(case))


@pytest.mark.parametrize("c0", PAIR_C0)
@pytest.mark.parametrize("case", PAIR_CASES, ids=pair_id)
def test_depth_pair_fill(P, case, c0):
    """[... c0 channels ... | p1 | p2 | 0 | 0]: each map against its own float64 resize, the pads zero, the channels in front untouched"""
    n, h, w, oh, ow = case
    p1, p2 = pair_inputs(case)
    f1, f2 = (P.Feat(p.reshape(n, h, w, 1).to(DEV)) for p in (p1, p2))
    dst = dst_feat(P, n, oh, ow, 4, c0, c0 + 4)
    P.depth_pair_fill(f1, f2, P.Feat(dst.buf, c0 + 2), c0)
    got = read(dst)
    for i, (p, ref) in enumerate(zip((p1, p2), pair_ref(case))):
        within(got[:, i:i + 1], ref, bilinear_tol(p), f"a depth_pair_fill map {i} c0={c0} {pair_id(case)}")
    assert bool((got[:, 2:] == 0).all()), "the pad channels must be zero"


# ---- b. roi_align: one map, fp32 output --------------------------------------------------------------------------------------------
# prv2_roi_align: vec as above; "rows" = roi_align_rows_kernel<4> (vec, oh >= 16), whose per-box branch is "one" sample per bin
# (gh == gw == 1) or the general "grid"; "pixel4" = roi_align_kernel<4> (vec, oh < 16); "scalar" = roi_align_kernel<1>.
# Boxes are (x1, y1, x2, y2) in multiples of 1/8, spatial_scale in {1.0, 0.5, 0.375}; the host file asserts for every box that no
# sampling coordinate is within 0.01 of -1 or of H (W) and that roi_h / oh, roi_w / ow are 0.01 away from every integer (the two places
# where the operation is discontinuous in the box; a degenerate box -- roi_w or roi_h <= 0 -- has no samples and is exempt).
MAP_A = dict(C=8, H=12, W=16, scale=0.5)     # image 32 x 24 at scale 0.5
MAP_B = dict(C=8, H=40, W=24, scale=1.0)
BOXES_A_ONE = [
    (4, 2, 20, 14),             # interior
    (0, 0, 8, 6),               # the top-left corner of the frame: samples in [-0.5, 0)
    (24, 18, 32, 24),           # ends exactly at the bottom-right corner
    (-3, -2.5, 9, 6.5),         # hangs over the top-left: samples in [-1, 0) and below -1
    (26, 20.5, 38, 30),         # hangs over the bottom-right: samples in (H - 1, H] and above H
]
BOXES_A_NARROW = [(4, 2, 11, 14), (-3, -2.25, 3.5, 6.5), (27, 20.5, 33.5, 30)]   # the same for 4 output columns (roi_w <= 4)
BOXES_B_GRID = [(0, 0, 24, 39.5), (-4, -6, 20.5, 37.5)]     # the second hangs over the top and the left edge
BOXES_A_MIXED = [(0, 0, 32, 24), (2, 1, 30, 23)]            # 16 x 5 outputs: gh = 1, gw = 4 and 3
DEGENERATE = [(12, 4, 12, 16), (4, 14, 20, 6)]              # zero width; negative height: no samples, rows of zeros
ROI_CASES = [
    dict(id="rows-one", **MAP_A, boxes=BOXES_A_ONE, out=(17, 22), path="rows/one"),                    # oh % 4 == 1
    dict(id="rows-grid", **MAP_B, boxes=BOXES_B_GRID, out=(16, 5), path="rows/grid"),                  # grid 3 x 5
    dict(id="rows-mixed", **MAP_A, boxes=BOXES_A_MIXED, out=(16, 5), path="rows/grid"),                # grid 1 x 4, 1 x 3
    dict(id="rows-grid-oh18", **MAP_B, boxes=BOXES_B_GRID, out=(18, 5), path="rows/grid"),             # py0 + r < oh false for two rows
    dict(id="pixel4-one", **MAP_A, boxes=BOXES_A_NARROW, out=(15, 4), path="pixel4/one"),
    dict(id="pixel4-grid", **MAP_B, boxes=BOXES_B_GRID, out=(5, 7), path="pixel4/grid"),
    dict(id="scalar-c3-one", **{**MAP_A, "C": 3}, boxes=BOXES_A_ONE, out=(17, 22), path="scalar/one"),
    dict(id="scalar-c1-grid", C=1, H=40, W=24, scale=0.375, boxes=[(0, 0, 64, 106), (8, 16, 50, 99)], out=(6, 5), path="scalar/grid"),
    dict(id="rows-degenerate", **MAP_A, boxes=DEGENERATE + BOXES_A_ONE[:1], out=(17, 22), path="rows/one", degenerate=True),
    dict(id="pixel4-degenerate", **MAP_A, boxes=DEGENERATE + BOXES_A_NARROW[:1], out=(15, 4), path="pixel4/one", degenerate=True),
    dict(id="scalar-degenerate", **{**MAP_A, "C": 3}, boxes=DEGENERATE + BOXES_A_ONE[:1], out=(17, 22), path="scalar/one", degenerate=True),
    dict(id="rows-one-slices", **MAP_A, boxes=BOXES_A_ONE, out=(17, 22), path="rows/one", layout="slice"),
]
ROI_BY_ID = {c["id"]: c for c in ROI_CASES}
ROI_BITEQ_CASES = ["rows-one", "rows-grid", "pixel4-grid"]     # again into a destination of pixel stride C + 1: roi_align_kernel<1>
ROI_X2_CASE = "pixel4-grid"                                     # roi_align_kernel<4, X2> with a grid above 1


def roi_layout(case, kind=None):
    """-> (c0 of the map, ld of the map, c0 of the output, ld of the output)"""
    c = case["C"]
    kind = kind or case.get("layout", "dense")
    return {"dense": (0, dense_ld(c), 0, dense_ld(c)), "slice": (4, c + 8, 8, c + 16), "odd": (0, dense_ld(c), 0, c + 1)}[kind]


def roi_input(case):
    return rnd(200 + ROI_CASES.index(ROI_BY_ID[case["id"]]), 1, case["C"], case["H"], case["W"])


def roi_geometry(box, scale, oh, ow, offset=0.5):
    """float64: -> (x1, y1, roi_w, roi_h, gh, gw) of torchvision's roi_align (aligned: offset 0.5), sampling_ratio = -1"""
    x1, y1, x2, y2 = (float(v) * scale - offset for v in box)
    rw, rh = x2 - x1, y2 - y1
    return x1, y1, rw, rh, math.ceil(rh / oh), math.ceil(rw / ow)


def roi_samples(box, scale, oh, ow, offset=0.5, grid=None):
    """-> [(yy [oh], xx [ow])] per sampling point of the gh x gw grid (float64); empty for a degenerate box"""
    x1, y1, rw, rh, gh, gw = roi_geometry(box, scale, oh, ow, offset)
    if grid is not None and rw > 0 and rh > 0:
        gh, gw = grid
    bh, bw = rh / oh, rw / ow
    ph, pw = torch.arange(oh, dtype=torch.float64), torch.arange(ow, dtype=torch.float64)
    return [(y1 + ph * bh + (iy + 0.5) * bh / gh, x1 + pw * bw + (ix + 0.5) * bw / gw) for iy in range(gh) for ix in range(gw)]


def roi_align64(feat, boxes, scale, oh, ow, offset=0.5, grid=None):
    """torchvision.ops.roi_align(aligned=True, sampling_ratio=-1) of ONE map [1, C, H, W], in float64 and without a tap of its own: every
    sampling point is F.grid_sample(bilinear, border, align_corners=True) at the pixel coordinates clamped to [0, H - 1] x [0, W - 1],
    times the validity mask not (y < -1 or y > H or x < -1 or x > W), averaged over the ceil(roi_h / oh) x ceil(roi_w / ow) grid
    (divisor max(count, 1)).  ``offset`` 0 is aligned=False, ``grid`` forces the sampling grid: the deliberately wrong variants"""
    _, C, H, W = feat.shape
    f = feat.double()
    res = []
    for box in boxes:
        pts = roi_samples(box, scale, oh, ow, offset, grid)
        acc = torch.zeros(C, oh, ow, dtype=torch.float64)
        for yy, xx in pts:
            valid = (~((yy < -1) | (yy > H)))[:, None] & (~((xx < -1) | (xx > W)))[None, :]
            gy = yy.clamp(0, H - 1) / (H - 1) * 2 - 1 if H > 1 else torch.zeros_like(yy)
            gx = xx.clamp(0, W - 1) / (W - 1) * 2 - 1 if W > 1 else torch.zeros_like(xx)
            grid_xy = torch.stack([gx[None, :].expand(oh, ow), gy[:, None].expand(oh, ow)], -1)[None]
            acc += F.grid_sample(f, grid_xy, mode="bilinear", padding_mode="border", align_corners=True)[0] * valid
        res.append(acc / max(len(pts), 1))
    return torch.stack(res)


@functools.lru_cache(maxsize=None)
def _roi_ref(cid):
    case = ROI_BY_ID[cid]
    return roi_align64(roi_input(case), case["boxes"], case["scale"], *case["out"])


def roi_ref(case):
    return _roi_ref(case["id"])


def roi_tol(case):
    """4 eps (H Dy + W Dx) + 8 eps max|x|: four roundings in a sampling coordinate (box * scale - 0.5, + p * bin, the in-bin offset, their
    sum), each at most eps / 2 of a magnitude <= 2 H (2 W); a coordinate error multiplies a neighbour difference.  Averaging over the grid
    does not increase the bound"""
    x = roi_input(case)
    dy, dx, mx = neighbour_diffs(x)
    return 4 * EPS * (case["H"] * dy + case["W"] * dx) + 8 * EPS * mx


def run_roi(P, case, kind=None, x2=False):
    oh, ow = case["out"]
    c0f, ldf, c0o, ldo = roi_layout(case, kind)
    boxes = torch.tensor(case["boxes"], dtype=torch.float32).to(DEV)
    out = dst_feat(P, len(case["boxes"]), oh, ow, case["C"], c0o, ldo)
    out.x2 = x2
    P.roi_align(src_feat(P, roi_input(case), c0f, ldf), boxes, case["scale"], oh, ow, out=out)
    return out


@pytest.mark.parametrize("case", ROI_CASES, ids=lambda c: c["id"])
def test_roi_align(P, case):
    got = read(run_roi(P, case))
    within(got, roi_ref(case), roi_tol(case), f"b roi_align {case['path']} {case['id']}")
    if case.get("degenerate"):
        assert float(roi_ref(case)[:2].abs().max()) == 0.0 and float(got[:2].abs().max()) == 0.0, "a box without samples gives zeros"


@pytest.mark.parametrize("cid", ROI_BITEQ_CASES)
def test_roi_align_kernels_agree_bit_for_bit(P, cid):
    case = ROI_BY_ID[cid]
    a, b = read(run_roi(P, case)), read(run_roi(P, case, "odd"))
    within(b, roi_ref(case), roi_tol(case), f"b roi_align scalar twin of {cid}")
    assert torch.equal(a, b)


def test_roi_align_x2_destination_per_pixel_grid(P):
    """the per-pixel kernel with a sampling grid above 1 writing the pre-split format: bf16 hi + bf16 lo of what the fp32 kernel writes"""
    case = ROI_BY_ID[ROI_X2_CASE]
    assert case["C"] % 8 == 0 and case["out"][0] < 16
    f32 = run_roi(P, case)
    got = run_roi(P, case, x2=True).x2_to_float().buf.cpu()
    v = f32.buf.cpu()
    hi = v.to(torch.bfloat16).float()
    want = hi + (v - hi).to(torch.bfloat16).float()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


# ---- c. crop_resize ------------------------------------------------------------------------------------------------------------------
CROP_IMG = (3, 40, 300)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (ch, cw, oh, ow, tiles (h0, w0), normalise): (0, 0), the exact bottom-right placement (H - ch, W - cw) and odd offsets
CROP_CASES = [
    (24, 280, 13, 270, ((0, 0), (16, 20), (7, 13)), True),      # 270 outputs per row: a second, partial block
    (10, 12, 23, 31, ((0, 0), (30, 288), (3, 5)), True),        # enlarges
    (40, 300, 1, 1, ((0, 0), (0, 0), (0, 0)), True),            # the whole image to one pixel
    (7, 9, 7, 9, ((5, 11), (33, 291), (0, 0)), False),          # identity, no mean / std: the pixels, bit for bit
]
CROP_LDO = (3, 4, 8)


def crop_id(c):
    return f"{c[0]}x{c[1]}-to-{c[2]}x{c[3]}"


def crop_image():
    return torch.rand(*CROP_IMG, generator=torch.Generator().manual_seed(300))


def crop_windows(case):
    ch, cw = case[:2]
    img = crop_image()
    return [img[:, h0:h0 + ch, w0:w0 + cw] for h0, w0 in case[4]]


def crop64(case, align_corners=True):
    wins = torch.stack(crop_windows(case)).double()
    v = F.interpolate(wins, case[2:4], mode="bilinear", align_corners=align_corners)
    if case[5]:
        v = (v - torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    return v


@functools.lru_cache(maxsize=None)
def crop_ref(case):
    return crop64(case)


def crop_tol(case):
    """the bilinear bound over the crop window (the largest of the tiles), divided by min(std), plus 4 eps max|ref| for the normalisation"""
    return max(bilinear_tol(win) for win in crop_windows(case)) / (min(STD) if case[5] else 1.0) + 4 * EPS * float(crop_ref(case).abs().max())


@pytest.mark.parametrize("ldo", CROP_LDO)
@pytest.mark.parametrize("case", CROP_CASES, ids=crop_id)
def test_crop_resize(P, case, ldo):
    ch, cw, oh, ow, tiles, norm = case
    out = dst_feat(P, len(tiles), oh, ow, 3, 0, ldo)
    P.crop_resize(crop_image().to(DEV), torch.tensor(tiles, dtype=torch.int32).to(DEV), ch, cw, oh, ow, MEAN if norm else None, STD if norm else None,
                  out)
    got = read(out)
    within(got, crop_ref(case), crop_tol(case), f"c crop_resize {crop_id(case)} ldo={ldo}")
    if (ch, cw) == (oh, ow) and not norm:
        assert torch.equal(got, torch.stack(crop_windows(case))), "the identity crop must copy the pixels"


# ---- d. ZoeDepth head ---------------------------------------------------------------------------------------------------------------------
MIN_TEMP, MAX_TEMP = 0.0212, 50.0
# (n, h, w, K, variant, layout).  prv2_zoe_logbinom_depth: "tile" = zoe_logbinom_depth_kernel<64> (K <= 64, 256 rows per block through an LDS
# tile), "generic" beyond.  Variants: "p" -- channel 0 (even pixels) or channel 1 (odd pixels) of pt is zero, p or 1 - p falls under 1e-4 and
# the clamp arms are taken; "t" -- channel 2 of pt is zero, the temperature is min_temp + 0.005 / pt[3], under 0.05 for most pixels.
# The trailing comment is d_ref, max|float32 restatement - float64 reference| on the CPU, of which the test allows four times
# (measured_tol); the test computes it where it runs, and a range is what two x86 hosts gave (torch's float32 log / exp differ with the
# host's vector unit); max|ref| is 8 .. 36
ZOE_CASES = [
    (2, 9, 31, 64, "plain", "dense"),       # 558 rows: two full blocks and a partial one            d_ref 1.11e-04
    (1, 16, 16, 64, "plain", "dense"),      # exactly one block                                      d_ref 2.24e-05 .. 4.63e-05
    (1, 1, 1, 64, "plain", "dense"),        #                                                        d_ref 4.85e-07 .. 9.62e-07
    (2, 9, 31, 16, "plain", "dense"),       # K < 64 on the tile kernel                              d_ref 5.64e-05 .. 5.83e-05
    (1, 5, 7, 2, "plain", "dense"),         #                                                        d_ref 1.57e-06
    (2, 9, 31, 65, "plain", "dense"),       # the generic kernel                                     d_ref 9.73e-05 .. 9.78e-05
    (1, 9, 11, 100, "plain", "dense"),      #                                                        d_ref 1.01e-04
    (2, 9, 31, 16, "p", "dense"),           #                                                        d_ref 1.26e-04
    (2, 9, 31, 16, "t", "dense"),           #                                                        d_ref 4.23e-04 .. 4.48e-04
    (2, 9, 31, 64, "p", "dense"),           #                                                        d_ref 2.69e-04
    (2, 9, 31, 64, "t", "dense"),           #                                                        d_ref 2.96e-03 .. 5.56e-03
    (1, 9, 11, 100, "p", "dense"),          #                                                        d_ref 1.16e-04
    (1, 9, 11, 100, "t", "dense"),          #                                                        d_ref 5.05e-03
    (2, 9, 31, 64, "plain", "slice"),       # pt = channels [4, 8) of 12, centers = [8, 72) of 80    d_ref 2.73e-04
]
# zoe_attractor (n_attr, n_bins) on 2 x 9 x 31 = 558 pixels; attr = channels [4, 4 + n_attr) of n_attr + 8, bins = channels [2, 2 + n_bins) of n_bins + 5
ATTR_CASES = [(16, 64), (1, 1), (300, 7), (8, 5)]      # d_ref 4.72e-07, 4.41e-07, 3.86e-07, 4.53e-07 (max|ref| 9 .. 12)
ATTR_PIXELS = (2, 9, 31)


def zoe_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-K{c[3]}-{c[4]}-{c[5]}"


def zoe_inputs(case):
    n, h, w, K, variant, _ = case
    i = ZOE_CASES.index(case)
    pt = F.softplus(rnd(400 + i, n, 4, h, w) * 2)
    centers = F.softplus(rnd(450 + i, n, K, h, w)) * 10
    if variant == "p":
        even = (torch.arange(n * h * w).view(n, h, w) % 2 == 0)
        pt[:, 0][even] = 0.0
        pt[:, 1][~even] = 0.0
    if variant == "t":
        pt[:, 2] = 0.0
    return pt, centers


def zoe_depth(pt, centers, dtype):
    """ConditionalLogBinomial's tail and the expectation of the bin centres (oracle/zoe.py: conditional_log_binomial, log_binom; zoedepth_forward)
    from the softplus outputs pt [n, 4, h, w] and the centres [n, K, h, w], evaluated in ``dtype``"""
    pt, centers = pt.to(dtype), centers.to(dtype)
    K = centers.shape[1]
    pp, t = pt[:, :2] + 1e-4, pt[:, 2:] + 1e-4
    x = (pp[:, 0] / (pp[:, 0] + pp[:, 1])).unsqueeze(1)
    t = (MAX_TEMP - MIN_TEMP) * (t[:, 0] / (t[:, 0] + t[:, 1])).unsqueeze(1) + MIN_TEMP
    one_minus = torch.clamp(1 - x, 1e-4, 1)
    x = torch.clamp(x, 1e-4, 1)
    k = torch.arange(0, K, dtype=dtype).view(1, -1, 1, 1)
    y = o_zoe.log_binom(torch.tensor([K - 1.0], dtype=dtype).view(1, -1, 1, 1), k) + k * torch.log(x) + (K - 1 - k) * torch.log(one_minus)
    return (torch.softmax(y / t, dim=1) * centers).sum(1, keepdim=True)


@functools.lru_cache(maxsize=None)
def zoe_ref(case):
    """-> (float64 reference, d_ref)"""
    pt, centers = zoe_inputs(case)
    ref = zoe_depth(pt, centers, torch.float64)
    return ref, float((zoe_depth(pt, centers, torch.float32).double() - ref).abs().max())


def measured_tol(ref, d_ref):
    """max(4 d_ref, 8 eps max|ref|): float32 divides the logits by a temperature as small as 0.02, and how far that alone takes a float32
    evaluation from float64 depends on the case -- so it is measured on the reference side (d_ref: torch float32 on the CPU against float64);
    4 x because the device's logf / expf are good to a couple of ulp where the CPU's are within one"""
    return max(4 * d_ref, 8 * EPS * float(ref.abs().max()))


@pytest.mark.parametrize("case", ZOE_CASES, ids=zoe_id)
def test_zoe_logbinom_depth(P, case):
    n, h, w, K, _, layout = case
    pt, centers = zoe_inputs(case)
    fp, fc = (src_feat(P, pt, 4, 12), src_feat(P, centers, 8, K + 16)) if layout == "slice" else (src_feat(P, pt, 0, 4), src_feat(P, centers, 0, roundup(K, 4)))
    got = P.zoe_logbinom_depth(fp, fc, MIN_TEMP, MAX_TEMP)
    ref, d_ref = zoe_ref(case)
    within(got, ref, measured_tol(ref, d_ref), f"d zoe_logbinom_depth {zoe_id(case)} (d_ref {d_ref:.2e})")


def attr_inputs(case):
    na, nb = case
    i = ATTR_CASES.index(case)
    return F.softplus(rnd(480 + i, ATTR_PIXELS[0], na, *ATTR_PIXELS[1:])), F.softplus(rnd(490 + i, ATTR_PIXELS[0], nb, *ATTR_PIXELS[1:])) * 3


def zoe_attract(attr, bins, dtype):
    """AttractorLayerUnnormed's tail, kind 'mean', type 'inv' (oracle/zoe.py: attractor_unnormed)"""
    a, b = attr.to(dtype), bins.to(dtype)
    return b + torch.mean(o_zoe.inv_attractor(a.unsqueeze(2) - b.unsqueeze(1)), dim=1)


@functools.lru_cache(maxsize=None)
def attr_ref(case):
    a, b = attr_inputs(case)
    ref = zoe_attract(a, b, torch.float64)
    return ref, float((zoe_attract(a, b, torch.float32).double() - ref).abs().max())


@pytest.mark.parametrize("case", ATTR_CASES, ids=lambda c: f"{c[0]}attr-{c[1]}bins")
def test_zoe_attractor(P, case):
    na, nb = case
    a, b = attr_inputs(case)
    out = P.zoe_attractor(src_feat(P, a, 4, na + 8), src_feat(P, b, 2, nb + 5), 300.0)
    assert (out.n, out.h, out.w, out.c) == (*ATTR_PIXELS, nb)
    ref, d_ref = attr_ref(case)
    within(out.buf[..., out.c0:out.c0 + nb].permute(0, 3, 1, 2), ref, measured_tol(ref, d_ref), f"d zoe_attractor {na} x {nb} (d_ref {d_ref:.2e})")


# ---- e. tokens and layout: exact ---------------------------------------------------------------------------------------------------------
PATCH_CASES = [(2, 2, 3, 14, 592), (1, 3, 2, 16, 768)]      # (b, gh, gw, p, ldo); 768 == 16 * 16 * 3: no pad columns
TOKEN_CASES = [(3, 6, 64), (1, 1, 8)]                       # (b, np, dim)
LAYOUT_SHAPES = [(2, 5, 3, 7), (1, 1, 1, 1)]                # (n, c, h, w), at ld = c and ld = c + 3


def patch_rows(img, p):
    """[b, 3, gh p, gw p] -> [b gh gw, p p 3]: row = (image, patch row, patch column), column = (ky, kx, channel)"""
    b, _, hh, ww = img.shape
    gh, gw = hh // p, ww // p
    return img.view(b, 3, gh, p, gw, p).permute(0, 2, 4, 3, 5, 1).reshape(b * gh * gw, p * p * 3)


@pytest.mark.parametrize("ld", [4, 3])
@pytest.mark.parametrize("case", PATCH_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-p{c[3]}-ldo{c[4]}")
def test_patchify(P, case, ld):
    b, gh, gw, p, ldo = case
    img = rnd(500, b, 3, gh * p, gw * p)
    rows = P.patchify(src_feat(P, img, 0, ld), p, ldo).cpu()
    assert rows.shape == (b * gh * gw, ldo)
    assert torch.equal(rows[:, :p * p * 3], patch_rows(img, p)) and bool((rows[:, p * p * 3:] == 0).all())


@pytest.mark.parametrize("case", TOKEN_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_assemble_tokens(P, case):
    b, np_, dim = case
    emb, cls, pos = rnd(510, b, np_, dim), rnd(511, 1, 1, dim), rnd(512, 1, np_ + 1, dim)
    tok = P.assemble_tokens(emb.reshape(b * np_, dim).to(DEV), cls.to(DEV), pos.to(DEV), b, np_, dim)
    assert torch.equal(tok.cpu(), torch.cat([cls.expand(b, -1, -1), emb], 1) + pos)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nchw_to_nhwc(P, shape, pad):
    """the entry point Feat.from_nchw calls (the wrapper chooses ld itself): pixel stride c + pad, the pad channels untouched"""
    n, c, h, w = shape
    x = rnd(520, *shape)
    xd, out = x.to(DEV), dst_feat(P, n, h, w, c, 0, c + pad)
    P._c("nchw_to_nhwc", xd.data_ptr(), n, c, h, w, out.ptr, out.ld)
    assert torch.equal(read(out), x)


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("shape", LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_nhwc_to_nchw(P, shape, pad):
    n, c, h, w = shape
    x = rnd(521, *shape)
    got = src_feat(P, x, pad // 2, c + pad).to_nchw()
    assert got.shape == x.shape and torch.equal(got.cpu(), x)


def test_add_three_strides(P):
    n, c, h, w = 2, 5, 3, 7
    a, b = rnd(530, n, c, h, w), rnd(531, n, c, h, w)
    out = dst_feat(P, n, h, w, c, 0, c + 2)
    P.add(src_feat(P, a, 1, c + 1), src_feat(P, b, 2, c + 4), out)
    assert torch.equal(read(out), a + b)


@pytest.mark.parametrize("pad", [0, 1, 3])
def test_zero_pad_channels(P, pad):
    """as Feat.alloc calls it: the live channels keep their contents, the pad channels become zero"""
    n, c, h, w = 2, 5, 3, 7
    before = rnd(540, n, h, w, c + pad)
    buf = before.to(DEV)
    if P.DISPATCH == "torch":
        P._tops().zero_pad_channels_(buf, c)
    else:
        P._c("zero_pad_channels", buf.data_ptr(), n * h * w, c, c + pad)
    got = buf.cpu()
    assert torch.equal(got[..., :c], before[..., :c]) and bool((got[..., c:] == 0).all())
