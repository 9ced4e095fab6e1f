"""CPU: the edge-aware evaluation's host spec (metrics.extract_edges / compute_boundary_metrics / edge_split_masks) against the
reference's own functions (tests/golden/edge_metrics.npz, tools/make_edge_golden.py), the dilation identity, and the ABI surface of
csrc/edges.hip (symbols, ops, argument checks) -- nothing here needs a GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "edge_metrics.npz")
NEW_SYMBOLS = ("prv2_edges_workspace_bytes", "prv2_depth_preprocess", "prv2_canny", "prv2_edt_sq", "prv2_binary_dilate", "prv2_boundary_stats")
NEW_OPS = ("depth_preprocess", "canny", "edt_sq", "binary_dilate", "boundary_stats")


def _golden():
    z = np.load(GOLDEN)
    return z, [str(c) for c in z["cases"]], [str(k) for k in z["metric_keys"]]


def test_extract_edges_matches_reference():
    from patchrefinerv2_amd import metrics as M
    z, cases, _ = _golden()
    assert len(cases) >= 5
    for c in cases:
        for mode in ("log", "inv", "none"):
            ref = z[f"{c}/gt_edges_{mode}"]
            got = M.extract_edges(z[f"{c}/gt"], preprocess=mode)
            assert got.dtype == bool and np.array_equal(got, ref), (c, mode, int((got != ref).sum()))
        assert np.array_equal(M.extract_edges(z[f"{c}/pred"], preprocess="log"), z[f"{c}/pred_edges_log"]), c
        assert np.array_equal(M.extract_edges(torch.from_numpy(z[f"{c}/gt"])[None, None], "log"), z[f"{c}/gt_edges_log"]), c


def test_compute_boundary_metrics_matches_reference():
    from patchrefinerv2_amd import metrics as M
    z, cases, keys = _golden()
    for c in cases:
        got = M.compute_boundary_metrics(z[f"{c}/gt_edges_log"], z[f"{c}/pred_edges_log"], z[f"{c}/valid"])
        assert list(got) == keys
        np.testing.assert_allclose([got[k] for k in keys], z[f"{c}/metrics"], rtol=1e-12, atol=0, err_msg=c)
    # the covered quirks: an empty prediction and no valid GT edge fall back to th; EdgeComp averages far GT edges too
    m = dict(zip(keys, z["empty_pred/metrics"]))
    assert m["EdgeAcc"] == 10 and m["EdgeComp"] == 10
    assert dict(zip(keys, z["edgecomp_quirk/metrics"]))["EdgeComp"] > 10


def test_extract_edges_rejects_mask_and_bad_mode():
    from patchrefinerv2_amd import metrics as M
    d = np.ones((8, 8), np.float32)
    with pytest.raises(NotImplementedError):
        M.extract_edges(d, "log", mask=np.ones((8, 8), bool))
    with pytest.raises(ValueError):
        M.extract_edges(d, "sqrt")


def _kornia_blur_positive(e, k):
    """kornia.filters.gaussian_blur2d(e, (k, k), (5, 5), 'reflect') > 0, restated"""
    i = torch.arange(k, dtype=torch.float32) - k // 2
    g = torch.exp(-(i ** 2) / 50.0)
    g = g / g.sum()
    x = torch.from_numpy(e.astype(np.float32))[None, None]
    x = F.pad(x, (k // 2,) * 4, mode="reflect")
    x = F.conv2d(F.conv2d(x, g.view(1, 1, 1, k)), g.view(1, 1, k, 1))
    return (x > 0)[0, 0].numpy()


@pytest.mark.parametrize("k", [5, 7])
def test_dilation_equals_kornia_blur_positive(k):
    from patchrefinerv2_amd import metrics as M
    rng = np.random.default_rng(k)
    for shape, p in (((40, 57), 0.01), ((23, 31), 0.1), ((9, 9), 0.05)):
        e = rng.random(shape) < p
        e[0, 0] = e[-1, -1] = True
        assert np.array_equal(M.binary_dilate(e, k), _kornia_blur_positive(e, k)), (shape, k)


def test_edge_split_masks_is_dilated_log_canny():
    from patchrefinerv2_amd import metrics as M
    z, cases, _ = _golden()
    gt = z[f"{cases[0]}/gt"]
    assert np.array_equal(M.edge_split_masks(gt), _kornia_blur_positive(z[f"{cases[0]}/gt_edges_log"], 7))


def test_gaussian_weights_are_scipys():
    from scipy import ndimage as ndi

    from patchrefinerv2_amd import metrics as M
    for sigma in (0.5, 1.0, 2.0):
        w = M.gaussian_weights(sigma)
        imp = np.zeros(41)
        imp[20] = 1.0
        ref = ndi.gaussian_filter1d(imp, sigma, mode="constant")
        assert np.array_equal(ref[20:20 + len(w)], w) and not ref[20 + len(w):].any()


def test_log_1_5_constant_is_torchs():
    from patchrefinerv2_amd import metrics as M
    assert M.LOG_1_5_F32 == torch.log(torch.tensor(1.5)).item()
    txt = open(os.path.join(ROOT, "patchrefinerv2_amd", "csrc", "edges.hip")).read()
    assert "0.405465096235275268554688f" in txt and float(np.float32(0.405465096235275268554688)) == M.LOG_1_5_F32


def test_abi_stays_20_and_new_symbols_are_bound():
    from patchrefinerv2_amd import lib as L
    hdr = open(os.path.join(ROOT, "include", "prv2.h")).read()
    assert "#define PRV2_ABI_VERSION 20" in hdr and L.ABI_VERSION == 20
    for s in NEW_SYMBOLS:
        assert s in L.SIGNATURES and f"{s}(" in hdr, s
    assert "edges.hip" in open(os.path.join(ROOT, "patchrefinerv2_amd", "csrc", "Makefile")).read()


def test_new_ops_reject_cpu_tensors():
    from patchrefinerv2_amd import torch_ops
    ops = torch_ops.load()
    for o in NEW_OPS:
        assert o in torch_ops.OPS
    f, b, i = torch.zeros(1, 8, 8), torch.zeros(1, 8, 8, dtype=torch.bool), torch.zeros(1, 8, 8, dtype=torch.int32)
    calls = [lambda: ops.depth_preprocess(f, 1), lambda: ops.canny(f, [0.5, 0.25], 0.1, 0.2), lambda: ops.edt_sq(b),
             lambda: ops.binary_dilate(b, 5), lambda: ops.boundary_stats(b, b, b, i, i, b, b, 10.0)]
    for c in calls:
        with pytest.raises((RuntimeError, NotImplementedError)):
            c()


def test_entry_points_reject_bad_arguments_without_gpu():
    import ctypes

    from patchrefinerv2_amd import lib as L
    lib = L.load()
    ws_need = lib.prv2_edges_workspace_bytes(2, 16, 24)
    assert ws_need > 2 * 16 * 24 * 4 * 8 and lib.prv2_edges_workspace_bytes(0, 16, 24) == -1
    w = np.array([0.5, 0.25], np.float64)
    P = 4096  # a non-null address that is never dereferenced: every call below fails its checks first

    def err(code):
        assert code != 0
        return lib.prv2_last_error()
    assert b"null" in err(lib.prv2_canny(None, 2, 16, 24, w.ctypes.data, 1, 0.1, 0.2, P, P, ws_need, None))
    assert b"null" in err(lib.prv2_canny(P, 2, 16, 24, None, 1, 0.1, 0.2, P, P, ws_need, None))
    assert b"3 x 3" in err(lib.prv2_canny(P, 2, 2, 24, w.ctypes.data, 1, 0.1, 0.2, P, P, ws_need, None))
    assert b"3 x 3" in err(lib.prv2_canny(P, 2, 16, 2, w.ctypes.data, 1, 0.1, 0.2, P, P, ws_need, None))
    assert b"workspace" in err(lib.prv2_canny(P, 2, 16, 24, w.ctypes.data, 1, 0.1, 0.2, P, P, ws_need - 1, None))
    assert b"workspace" in err(lib.prv2_canny(P, 2, 16, 24, w.ctypes.data, 1, 0.1, 0.2, P, None, ws_need, None))
    assert b"radius" in err(lib.prv2_canny(P, 2, 16, 24, w.ctypes.data, 16, 0.1, 0.2, P, P, ws_need, None))
    assert b"null" in err(lib.prv2_depth_preprocess(None, 2, 16, 24, 1, P, P, ws_need, None))
    assert b"mode" in err(lib.prv2_depth_preprocess(P, 2, 16, 24, 7, P, P, ws_need, None))
    assert b"workspace" in err(lib.prv2_depth_preprocess(P, 2, 16, 24, 2, P, P, 64, None))
    assert b"3 x 3" in err(lib.prv2_depth_preprocess(P, 2, 16, 1, 1, P, P, ws_need, None))
    assert b"null" in err(lib.prv2_edt_sq(P, 2, 16, 24, None, P, ws_need, None))
    assert b"workspace" in err(lib.prv2_edt_sq(P, 2, 16, 24, P, P, 0, None))
    assert b"3 x 3" in err(lib.prv2_edt_sq(P, 2, 0, 24, P, P, ws_need, None))
    assert b"width" in err(lib.prv2_edt_sq(P, 1, 3, 6000, P, P, lib.prv2_edges_workspace_bytes(1, 3, 6000), None))
    assert b"null" in err(lib.prv2_binary_dilate(None, 2, 16, 24, 5, P, None))
    assert b"k = 4" in err(lib.prv2_binary_dilate(P, 2, 16, 24, 4, P, None))
    assert b"3 x 3" in err(lib.prv2_binary_dilate(P, 2, 16, -3, 5, P, None))
    assert b"null" in err(lib.prv2_boundary_stats(P, P, None, P, P, P, P, 2, 16, 24, 10.0, P, P, ws_need, None))
    assert b"null" in err(lib.prv2_boundary_stats(P, P, P, P, P, P, P, 2, 16, 24, 10.0, None, P, ws_need, None))
    assert b"workspace" in err(lib.prv2_boundary_stats(P, P, P, P, P, P, P, 2, 16, 24, 10.0, P, P, ws_need // 2, None))
    assert b"frame count" in err(lib.prv2_boundary_stats(P, P, P, P, P, P, P, 0, 16, 24, 10.0, P, P, ws_need, None))
    assert ctypes.sizeof(ctypes.c_double) == 8


def test_image_dataset_edge_metrics_host_route(tmp_path):
    """ImageDataset(edge_metrics=True).get_metrics on CPU tensors: the host route adds the boundary metrics and edge_/noedge_ splits"""
    from patchrefinerv2_amd import metrics as M
    from patchrefinerv2_amd.tester import ImageDataset
    (tmp_path / "rgb").mkdir()
    z, cases, keys = _golden()
    gt = torch.from_numpy(z[f"{cases[0]}/gt"])[None, None]
    pred = torch.from_numpy(z[f"{cases[0]}/pred"])[None, None]
    plain = ImageDataset(str(tmp_path / "rgb"), min_depth=0.1, max_depth=10).get_metrics(gt, pred)
    ds = ImageDataset(str(tmp_path / "rgb"), min_depth=0.1, max_depth=10, edge_metrics=True)
    m = ds.get_metrics(gt, pred)
    for k, v in plain.items():
        assert m[k] == v and f"edge_{k}" in m and f"noedge_{k}" in m
    ref = M.compute_boundary_metrics(z[f"{cases[0]}/gt_edges_log"], z[f"{cases[0]}/pred_edges_log"], (gt > 0.1) & (gt < 10))
    for k in keys:
        assert m[k] == ref[k], k
    region = torch.from_numpy(M.edge_split_masks(gt))
    e = M.compute_metrics(gt, pred, garg_crop=False, eigen_crop=False, min_depth_eval=0.1, max_depth_eval=10, additional_mask=region)
    assert all(m[f"edge_{k}"] == v for k, v in e.items())
