"""CPU side of tests/test_resample_kernels_gpu.py: its tables, float64 references and tolerances are sound before any kernel runs -- every
row is valid and takes the launch path it names (a restatement of the launchers' predicates in csrc/gather.hip and csrc/pointwise.hip),
the float32 oracle of every row stays inside the row's tolerance (inside half of it for the derived bounds), a deliberately wrong
float64 variant misses the reference by 100 tolerances, and the ROI boxes keep their distance from the two places where roi_align is
discontinuous in the box.  Nothing here loads the library."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_resample_kernels_gpu as G
from oracle import ops as o_ops


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max())


def gather_path(c, ldx, ldy, oh):
    """prv2_upsample_bilinear / roi_align_impl; the buffers are torch allocations and the slices start at multiples of 4 channels, so the
    16-byte alignment of the predicate holds whenever the strides allow it"""
    vec = c % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0
    return "rows" if vec and oh >= 16 else "pixel4" if vec else "scalar"


# ---- a. bilinear --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.UP_CASES, ids=G.up_id)
def test_upsample_case(case):
    n, c, h, w, oh, ow, path = case
    x, ref, tol = G.up_input(case), G.up_ref(case), G.bilinear_tol(G.up_input(case))
    assert ref.shape == (n, c, oh, ow) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    assert G.up_ref(case) is ref    # computed once
    c0x, ldx, c0y, ldy = G.up_layout(case, "dense")
    assert path == gather_path(c, ldx, ldy, oh) and c0x + c <= ldx and c0y + c <= ldy
    assert maxdiff(o_ops.bilinear_ac(x, (oh, ow)), ref) <= 0.5 * tol                       # the float32 oracle alone stays inside the limit
    assert maxdiff(o_ops.bilinear_ac_explicit(x, (oh, ow)), ref) <= 0.5 * tol              # ... and the index-level restatement of the kernels' rule
    if (h, w) != (oh, ow):
        assert maxdiff(G.bilinear64(x, oh, ow, align_corners=False), ref) >= 100 * tol


@pytest.mark.parametrize("hw", [(56, 84, 28, 42), (97, 130, 33, 65)])
def test_bilinear_bound_at_larger_sizes(hw):
    """the derivation does not lean on the small sizes of the table"""
    h, w, oh, ow = hw
    x = G.rnd(150, 1, 4, h, w)
    assert maxdiff(o_ops.bilinear_ac(x, (oh, ow)), G.bilinear64(x, oh, ow)) <= 0.5 * G.bilinear_tol(x)


def test_upsample_cases_take_the_paths_they_name():
    rows = [c for c in G.UP_CASES if c[6] == "rows"]
    px = [c for c in G.UP_CASES if c[6] == "pixel4"]
    assert len({G.up_id(c) for c in G.UP_CASES}) == len(G.UP_CASES)
    assert {c[4] % 4 for c in rows} >= {1, 2, 3}                                           # the tail of the last block of rows: every length
    assert any(c[2] > 2 * c[4] for c in rows)                                              # down-sampling by more than 2: both cache entries miss
    assert any(c[2] == 1 for c in rows) and any(c[3] == 1 for c in rows) and any(c[2:4] == c[4:6] for c in rows)
    assert any(c[4:6] == (1, 1) for c in px) and any(c[4] == 1 < c[5] for c in px) and any(c[5] == 1 < c[4] for c in px)
    assert all(c[4] < 16 for c in px) and {c[1] for c in G.UP_CASES if c[6] == "scalar"} == {3, 1}
    assert any((c[4] + 3) // 4 > 1 for c in rows) and any(c[0] > 1 for c in rows)          # several blocks of rows, several images
    # slices: one rows case and one per-pixel case, each still on its kernel; both slices leave NaN / sentinel neighbours on either side
    assert [c[6] for c in G.UP_SLICE_CASES] == ["rows", "pixel4"]
    for case in G.UP_SLICE_CASES:
        c0x, ldx, c0y, ldy = G.up_layout(case, "slice")
        assert case[6] == gather_path(case[1], ldx, ldy, case[4]) and c0x % 4 == 0 and c0y % 4 == 0
        assert 0 < c0x and c0x + case[1] < ldx and 0 < c0y and c0y + case[1] < ldy
    # bit equality: two rows cases (one of them down-sampling), one per-pixel case, each against upsample_bilinear_kernel<1>
    assert [c[6] for c in G.UP_BITEQ_CASES] == ["rows", "rows", "pixel4"] and any(c[2] > c[4] for c in G.UP_BITEQ_CASES)
    for case in G.UP_BITEQ_CASES:
        c0x, ldx, c0y, ldy = G.up_layout(case, "odd")
        assert ldy == case[1] + 1 and gather_path(case[1], ldx, ldy, case[4]) == "scalar"


@pytest.mark.parametrize("case", G.PAIR_CASES, ids=G.pair_id)
def test_depth_pair_case(case):
    n, h, w, oh, ow = case
    assert all(c0 % 4 == 0 for c0 in G.PAIR_C0) and 0 in G.PAIR_C0 and any(G.PAIR_C0)
    for p, ref in zip(G.pair_inputs(case), G.pair_ref(case)):
        tol = G.bilinear_tol(p)
        assert ref.shape == (n, 1, oh, ow) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
        assert maxdiff(o_ops.bilinear_ac(p, (oh, ow)), ref) <= 0.5 * tol
        assert maxdiff(G.bilinear64(p, oh, ow, align_corners=False), ref) >= 100 * tol
    assert not torch.equal(*G.pair_inputs(case))    # two different maps: a swap of the two channels shows


# ---- b. roi_align ---------------------------------------------------------------------------------------------------------------------------
MARGIN = 0.01


def grid_f32(box, scale, oh, ow):
    """(gh, gw) as the kernels take them: float32 throughout, ceilf of the float32 quotient"""
    f = np.float32
    x1, y1, x2, y2 = (f(v) * f(scale) - f(0.5) for v in box)
    return int(np.ceil(f(y2 - y1) / f(oh))), int(np.ceil(f(x2 - x1) / f(ow)))


def live_boxes(case):
    """the boxes with samples (roi_w > 0 and roi_h > 0)"""
    return [b for b in case["boxes"] if min(G.roi_geometry(b, case["scale"], *case["out"])[2:4]) > 0]


def sample_coords(case, box):
    """-> (all y coordinates, all x coordinates) of a box's sampling points, float64"""
    pts = G.roi_samples(box, case["scale"], *case["out"])
    return torch.cat([p[0] for p in pts]), torch.cat([p[1] for p in pts])


@pytest.mark.parametrize("case", G.ROI_CASES, ids=lambda c: c["id"])
def test_roi_case(case):
    C, H, W, scale, (oh, ow) = case["C"], case["H"], case["W"], case["scale"], case["out"]
    kernel, branch = case["path"].split("/")
    x, ref, tol = G.roi_input(case), G.roi_ref(case), G.roi_tol(case)
    assert ref.shape == (len(case["boxes"]), C, oh, ow) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    assert G.roi_ref(case) is ref
    assert scale in (1.0, 0.5, 0.375) and all(float(v) * 8 == int(float(v) * 8) for b in case["boxes"] for v in b)
    c0f, ldf, c0o, ldo = G.roi_layout(case)
    assert kernel == gather_path(C, ldf, ldo, oh) and c0f + C <= ldf and c0o + C <= ldo
    live = live_boxes(case)
    assert len(live) == len(case["boxes"]) - (2 if case.get("degenerate") else 0) and live
    for box in case["boxes"]:
        x1, y1, rw, rh, gh, gw = G.roi_geometry(box, scale, oh, ow)
        assert (max(gh, 0), max(gw, 0)) == tuple(max(g, 0) for g in grid_f32(box, scale, oh, ow))       # float64 ceil == the kernels' float32 ceilf
        if box not in live:
            assert gh * gw <= 0 and not G.roi_samples(box, scale, oh, ow)
            continue
        # the launch branch: one sample per bin iff gh == gw == 1 (the rows kernel's general branch iff gh != 1 or gw != 1)
        assert ((gh, gw) == (1, 1)) == (branch == "one"), (box, gh, gw)
        # discontinuity 2: the sampling grid's size -- the bin sizes keep away from every integer
        for q in (rh / oh, rw / ow):
            assert abs(q - round(q)) >= MARGIN, (box, q)
        # discontinuity 1: the validity mask -- no sampling coordinate near -1 or near H (W)
        yy, xx = sample_coords(case, box)
        for v, size in ((yy, H), (xx, W)):
            assert float(torch.minimum((v + 1).abs(), (v - size).abs()).min()) >= MARGIN, (box, size)
    # soundness: the float32 restatement of torchvision's kernel stays inside half of the tolerance
    rois = torch.tensor([[0.0, *map(float, b)] for b in case["boxes"]])
    assert maxdiff(o_ops.roi_align(x, rois, (oh, ow), scale, aligned=True), ref) <= 0.5 * tol
    # discrimination: aligned=False (no -0.5), and for the grid rows a sampling grid forced to 1 x 1
    assert maxdiff(G.roi_align64(x, case["boxes"], scale, oh, ow, offset=0.0), ref) >= 100 * tol
    if branch == "grid":
        assert maxdiff(G.roi_align64(x, case["boxes"], scale, oh, ow, grid=(1, 1)), ref) >= 100 * tol
    if case.get("degenerate"):
        assert float(ref[:2].abs().max()) == 0.0 and float(ref[2].abs().min()) > 0.0


def test_roi_cases_take_the_paths_they_name():
    ids = [c["id"] for c in G.ROI_CASES]
    assert len(set(ids)) == len(ids)
    by_path = {}
    for c in G.ROI_CASES:
        by_path.setdefault(c["path"], []).append(c)
    assert set(by_path) == {"rows/one", "rows/grid", "pixel4/one", "pixel4/grid", "scalar/one", "scalar/grid"}
    grids = {c["id"]: [G.roi_geometry(b, c["scale"], *c["out"])[4:] for b in live_boxes(c)] for c in G.ROI_CASES}
    # the rows kernel's general branch: a full grid, the mixed one (one sample down, several across), and an output height that is no multiple of 4
    assert (3, 5) in grids["rows-grid"] and any(gh == 1 < gw for gh, gw in grids["rows-mixed"])
    assert any(c["out"][0] % 4 == 2 and c["out"][0] >= 16 for c in by_path["rows/grid"])
    assert any(c["out"][0] % 4 == 1 for c in by_path["rows/one"])                          # py < oh false in the one-sample branch, too
    assert all(max(gh * gw for gh, gw in grids[c["id"]]) > 1 for p in ("pixel4/grid", "scalar/grid") for c in by_path[p])
    assert {c["C"] for c in by_path["scalar/one"] + by_path["scalar/grid"]} == {3, 1}
    # samples in the clamped bands [-1, 0) and (H - 1, H] (and their x twins), and samples beyond them that the mask drops
    for kernel in ("rows", "pixel4", "scalar"):
        lo = hi = out_lo = out_hi = False
        for c in G.ROI_CASES:
            if not c["path"].startswith(kernel):
                continue
            for box in live_boxes(c):
                yy, xx = sample_coords(c, box)
                for v, size in ((yy, c["H"]), (xx, c["W"])):
                    lo |= bool(((v >= -1) & (v < 0)).any())
                    hi |= bool(((v > size - 1) & (v <= size)).any())
                    out_lo |= bool((v < -1).any())
                    out_hi |= bool((v > size).any())
        assert lo and out_lo and hi and out_hi, (kernel, lo, hi, out_lo, out_hi)
    # a box ending exactly at the bottom-right corner of the frame, one starting at its top-left corner
    a = G.ROI_BY_ID["rows-one"]
    assert any(b[2] * a["scale"] == a["W"] and b[3] * a["scale"] == a["H"] for b in a["boxes"]) and any(b[:2] == (0, 0) for b in a["boxes"])
    # one degenerate row per kernel: a zero-width and a negative-height box beside a normal one
    deg = [c for c in G.ROI_CASES if c.get("degenerate")]
    assert sorted(c["path"].split("/")[0] for c in deg) == ["pixel4", "rows", "scalar"]
    for c in deg:
        (_, _, rw0, rh0, *_), (_, _, rw1, rh1, *_) = (G.roi_geometry(b, c["scale"], *c["out"]) for b in c["boxes"][:2])
        assert rw0 == 0 and rh0 > 0 and rw1 > 0 and rh1 < 0
    # the slice row: on the rows kernel, neighbours on both sides of both slices
    s = [c for c in G.ROI_CASES if c.get("layout") == "slice"]
    assert len(s) == 1 and s[0]["path"].startswith("rows")
    c0f, ldf, c0o, ldo = G.roi_layout(s[0])
    assert 0 < c0f and c0f + s[0]["C"] < ldf and 0 < c0o and c0o + s[0]["C"] < ldo


def test_roi_references_are_not_tests_of_zeros():
    nz = tot = 0
    for c in G.ROI_CASES:
        if not c.get("degenerate"):
            nz, tot = nz + int((G.roi_ref(c) != 0).sum()), tot + G.roi_ref(c).numel()
    assert nz >= 0.7 * tot, nz / tot


def test_roi_bit_equality_and_x2_rows():
    assert [G.ROI_BY_ID[i]["path"] for i in G.ROI_BITEQ_CASES] == ["rows/one", "rows/grid", "pixel4/grid"]
    for cid in G.ROI_BITEQ_CASES:
        c = G.ROI_BY_ID[cid]
        c0f, ldf, c0o, ldo = G.roi_layout(c, "odd")
        assert ldo == c["C"] + 1 and gather_path(c["C"], ldf, ldo, c["out"][0]) == "scalar"
    x2 = G.ROI_BY_ID[G.ROI_X2_CASE]
    assert x2["path"] == "pixel4/grid" and x2["C"] % 8 == 0 and x2["out"][0] < 16 and G.roi_layout(x2)[3] % 8 == 0


def test_roi_reference_is_the_plain_definition():
    """roi_align64 against a direct float64 evaluation of the definition (own floor / weights) on one interior grid box: the grid_sample
    formulation samples where it should"""
    case = G.ROI_BY_ID["pixel4-grid"]
    x, (oh, ow), box = G.roi_input(case).double()[0], case["out"], case["boxes"][0]
    x1, y1, rw, rh, gh, gw = G.roi_geometry(box, case["scale"], oh, ow)
    want = torch.zeros(case["C"], oh, ow, dtype=torch.float64)
    for py in range(oh):
        for px in range(ow):
            for iy in range(gh):
                for ix in range(gw):
                    y = min(max(y1 + py * rh / oh + (iy + 0.5) * rh / oh / gh, 0.0), case["H"] - 1.0)
                    xx = min(max(x1 + px * rw / ow + (ix + 0.5) * rw / ow / gw, 0.0), case["W"] - 1.0)
                    y0, x0 = min(int(y), case["H"] - 2), min(int(xx), case["W"] - 2)
                    ly, lx = y - y0, xx - x0
                    want[:, py, px] += ((1 - ly) * (1 - lx) * x[:, y0, x0] + (1 - ly) * lx * x[:, y0, x0 + 1] + ly * (1 - lx) * x[:, y0 + 1, x0]
                                        + ly * lx * x[:, y0 + 1, x0 + 1]) / (gh * gw)
    assert maxdiff(G.roi_ref(case)[0], want) <= 1e-12


# ---- c. crop_resize -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.CROP_CASES, ids=G.crop_id)
def test_crop_case(case):
    ch, cw, oh, ow, tiles, norm = case
    _, H, W = G.CROP_IMG
    ref, tol = G.crop_ref(case), G.crop_tol(case)
    assert ref.shape == (len(tiles), 3, oh, ow) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    assert len(tiles) >= 3 and all(0 <= h0 <= H - ch and 0 <= w0 <= W - cw for h0, w0 in tiles)
    assert (0, 0) in tiles and (H - ch, W - cw) in tiles
    # the float32 oracle: torch's float32 resize of the crop, normalised in float32
    v = o_ops.bilinear_ac(torch.stack(G.crop_windows(case)), (oh, ow))
    if norm:
        v = (v - torch.tensor(G.MEAN).view(1, 3, 1, 1)) / torch.tensor(G.STD).view(1, 3, 1, 1)
    assert maxdiff(v, ref) <= 0.5 * tol
    if (ch, cw) != (oh, ow):
        assert maxdiff(G.crop64(case, align_corners=False), ref) >= 100 * tol
    else:
        assert not norm and torch.equal(ref.float(), torch.stack(G.crop_windows(case))) and any(h0 and w0 for h0, w0 in tiles)


def test_crop_cases_cover_what_they_name():
    assert any(c[3] > 256 and c[3] % 256 for c in G.CROP_CASES)                            # a second, partial block along the row
    assert any(c[2] > c[0] and c[3] > c[1] for c in G.CROP_CASES)                          # enlarging
    assert any(c[2:4] == (1, 1) and c[:2] == G.CROP_IMG[1:] for c in G.CROP_CASES)
    assert any(h0 % 2 and w0 % 2 for c in G.CROP_CASES for h0, w0 in c[4])                 # odd offsets
    assert set(G.CROP_LDO) == {3, 4, 8}


# ---- d. ZoeDepth head -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.ZOE_CASES, ids=G.zoe_id)
def test_zoe_case(case):
    n, h, w, K, variant, layout = case
    pt, centers = G.zoe_inputs(case)
    ref, d_ref = G.zoe_ref(case)
    assert ref.shape == (n, 1, h, w) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    assert bool(torch.isfinite(G.zoe_depth(pt, centers, torch.float32)).all())
    assert K > 1 and pt.dtype == centers.dtype == torch.float32 and float(pt.min()) >= 0 and float(centers.min()) > 0
    # the expectation of the centres lies between them
    assert bool((ref[:, 0] >= centers.double().min(1).values - 1e-9).all()) and bool((ref[:, 0] <= centers.double().max(1).values + 1e-9).all())
    # the float32 restatement alone stays inside the limit
    assert d_ref <= G.measured_tol(ref, d_ref) and G.measured_tol(ref, d_ref) <= 0.05 * float(ref.abs().max())
    print(f"d_ref {G.zoe_id(case)} = {d_ref:.2e} (max|ref| {float(ref.abs().max()):.2f})")
    p = (pt[:, 0].double() + 1e-4) / (pt[:, 0].double() + pt[:, 1].double() + 2e-4)
    t = (G.MAX_TEMP - G.MIN_TEMP) * (pt[:, 2].double() + 1e-4) / (pt[:, 2].double() + pt[:, 3].double() + 2e-4) + G.MIN_TEMP
    if variant == "p":      # both clamp arms: p under 1e-4 somewhere, 1 - p under 1e-4 somewhere else
        assert bool((p < 1e-4).any()) and bool((1 - p < 1e-4).any())
    else:
        assert bool(((p > 1e-4) & (1 - p > 1e-4)).all())
    if variant == "t":
        assert float(t.median()) < 0.05 and float(t.min()) >= G.MIN_TEMP
    else:
        assert float(t.median()) > 1.0


def test_zoe_cases_take_the_paths_they_name():
    tile = lambda c: c[3] <= 64    # noqa: E731  (prv2_zoe_logbinom_depth: the LDS-tile kernel up to 64 bins, the generic one beyond)
    rows = lambda c: c[0] * c[1] * c[2]    # noqa: E731
    plain = [c for c in G.ZOE_CASES if c[4] == "plain" and c[5] == "dense"]
    assert len({G.zoe_id(c) for c in G.ZOE_CASES}) == len(G.ZOE_CASES)
    assert any(tile(c) and c[3] == 64 and rows(c) > 512 and rows(c) % 256 for c in plain)  # full blocks, then a partial one
    assert any(tile(c) and rows(c) == 256 for c in plain) and any(tile(c) and rows(c) == 1 for c in plain)
    assert any(tile(c) and 2 < c[3] < 64 and rows(c) > 256 for c in plain) and any(c[3] == 2 for c in plain)
    assert any(c[3] == 65 and rows(c) > 256 and rows(c) % 256 for c in plain) and any(c[3] > 65 for c in plain)
    for v in ("p", "t"):
        assert {c[3] for c in G.ZOE_CASES if c[4] == v} == {16, 64, 100}
    assert [c[3] for c in G.ZOE_CASES if c[5] == "slice"] == [64]


@pytest.mark.parametrize("case", G.ATTR_CASES, ids=lambda c: f"{c[0]}attr-{c[1]}bins")
def test_attractor_case(case):
    na, nb = case
    a, b = G.attr_inputs(case)
    ref, d_ref = G.attr_ref(case)
    n, h, w = G.ATTR_PIXELS
    assert ref.shape == (n, nb, h, w) and ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    assert n * h * w * nb > 256 and (n * h * w * nb) % 256                                 # more than one block, the last partial
    assert d_ref <= G.measured_tol(ref, d_ref) <= 1e-4 * float(ref.abs().max())
    print(f"d_ref attractor {na} x {nb} = {d_ref:.2e} (max|ref| {float(ref.abs().max()):.2f})")
    # the definition, pixel by pixel and bin by bin
    a64, b64 = a.double(), b.double()
    want = torch.stack([b64[:, j] + sum((a64[:, i] - b64[:, j]) / (1 + 300.0 * (a64[:, i] - b64[:, j]) ** 2) for i in range(na)) / na for j in range(nb)], 1)
    assert maxdiff(ref, want) <= 1e-12
    assert maxdiff(ref, b64) > 100 * G.measured_tol(ref, d_ref)                            # the attractors move the bins


# ---- e. tokens and layout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.PATCH_CASES)
def test_patch_rows_is_unfold(case):
    b, gh, gw, p, ldo = case
    img = G.rnd(500, b, 3, gh * p, gw * p)
    u = F.unfold(img, p, stride=p)                                                         # [b, (c, ky, kx), gh gw]
    want = u.view(b, 3, p, p, gh * gw).permute(0, 4, 2, 3, 1).reshape(b * gh * gw, p * p * 3)
    assert torch.equal(G.patch_rows(img, p), want) and ldo >= p * p * 3
    assert G.patch_rows(img, p)[gw + 1, (2 * p + 3) * 3 + 1] == img[0, 1, p + 2, p + 3]    # patch (1, 1), pixel (2, 3), channel 1


def test_token_and_layout_tables():
    assert any(c[4] > c[3] * c[3] * 3 for c in G.PATCH_CASES) and any(c[4] == c[3] * c[3] * 3 for c in G.PATCH_CASES)
    assert (3, 6, 64) in G.TOKEN_CASES and (1, 1, 8) in G.TOKEN_CASES
    assert (2, 5, 3, 7) in G.LAYOUT_SHAPES and (1, 1, 1, 1) in G.LAYOUT_SHAPES


def test_gpu_file_is_marked():
    assert G.pytestmark.name == "gpu" and math.isclose(G.EPS, 2.0 ** -23)
