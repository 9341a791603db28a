"""CPU checks of the frame metrics (unboundednerfpytorch_amd.metrics, csrc/ugrid_metrics.hip): the numpy statement of the formula
against the reference's own maps, the C ABI's host-side halves (workspace size, refusals before the device is touched), the
argument errors of the Python layers and the kernel's register metadata.  The kernel itself runs in test_gpu_metrics.py."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import metrics_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from unboundednerfpytorch_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden_maps(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ssim_maps.npz")))


@pytest.mark.parametrize("name", list(metrics_cases.PAIRS))
def test_numpy_formula_matches_the_reference_maps(name, golden_maps):
    """the golden-free numpy implementation of tests/metrics_cases.py = the reference's utils.rgb_ssim(..., return_map=True)"""
    img, gt = metrics_cases.pair(name)
    gold = golden_maps[name]
    assert gold.dtype == np.float64 and gold.shape == (img.shape[0] - 10, img.shape[1] - 10, 3)
    m = metrics_cases.ssim_map_numpy(img, gt)
    assert np.abs(m - gold).max() <= 1e-12
    assert abs(m.mean() - gold.mean()) <= 1e-12
    if name == "identical":
        assert (gold == 1.0).all() and metrics_cases.sq_err_sum_numpy(img, gt) == 0.0
    if name == "negated":
        assert gold.max() < 0.0


def test_pairs_cover_the_tile_edges():
    """map extents T-1, T, T+1 and 2T+3 on each axis of the kernel's 32 x 54 tile, a 1 x 1 map, and more than one workgroup"""
    from unboundednerfpytorch_amd import metrics
    assert (metrics.TILE_Y, metrics.TILE_X) == (metrics_cases.TILE_Y, metrics_cases.TILE_X)
    rows = {p[2] - 10 for p in metrics_cases.PAIRS.values()}
    cols = {p[3] - 10 for p in metrics_cases.PAIRS.values()}
    for T, have in ((metrics.TILE_Y, rows), (metrics.TILE_X, cols)):
        assert {T - 1, T, T + 1, 2 * T + 3} <= have
    assert 1 in rows and 1 in cols


def test_symbols_and_workspace_layout(lib):
    from unboundednerfpytorch_amd import _lib, metrics
    assert "ugrid_frame_metrics" in _lib.EXPORTED_SYMBOLS and "ugrid_frame_metrics_ws_bytes" in _lib.EXPORTED_SYMBOLS
    assert lib.ugrid_abi_version() == _lib.ABI_VERSION == 3
    # one {squared error, ssim} pair of doubles per 32 x 54 tile of the [(H-10),(W-10)] map; nothing for a frame it refuses
    ceil = lambda a, b: -(-a // b)
    for H, W in ((11, 11), (13, 75), (42, 64), (43, 65), (77, 121), (1080, 1920), (2160, 3840)):
        want = 16 * ceil(H - 10, 32) * ceil(W - 10, 54)
        assert lib.ugrid_frame_metrics_ws_bytes(H, W) == want == metrics.workspace_bytes(H, W)
    assert lib.ugrid_frame_metrics_ws_bytes(1080, 1920) == 16 * 34 * 36
    assert lib.ugrid_frame_metrics_ws_bytes(10, 64) == 0 and lib.ugrid_frame_metrics_ws_bytes(64, 10) == 0


def test_entry_point_refuses_before_touching_the_device(lib):
    """H < 11, W < 11 and filter_size != 11 -> hipErrorInvalidValue (1) on a machine without a device: the pointers are never
    dereferenced and nothing is launched"""
    fake = ctypes.c_void_p(0x1000)

    def call(H, W, fs):
        return lib.ugrid_frame_metrics(fake, 3, fake, 3, H, W, fs, 1.5, 0.01, 0.03, 1.0, fake, None, fake, None)
    assert call(10, 64, 11) == 1
    assert call(64, 10, 11) == 1
    assert call(64, 64, 9) == 1
    assert call(64, 64, 13) == 1


def test_frame_metrics_argument_errors():
    from unboundednerfpytorch_amd import metrics
    a = torch.zeros(16, 16, 3)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        metrics.frame_metrics(a, a)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        metrics.frame_metrics(a.reshape(-1, 3), a.reshape(-1, 3), H=16, W=16)
    with pytest.raises(ValueError):
        metrics.rgb_ssim(np.zeros((16, 16, 3), np.float32), np.zeros((16, 17, 3), np.float32), 1.0)
    import inspect
    names = list(inspect.signature(metrics.rgb_ssim).parameters)
    assert names == ["img0", "img1", "max_val", "filter_size", "filter_sigma", "k1", "k2", "return_map"]   # utils.py:79-84
    assert list(inspect.signature(metrics.frame_metrics).parameters)[:5] == ["img", "gt", "max_val", "return_map", "out"]


def test_sums_to_psnr_and_mean_ssim():
    from unboundednerfpytorch_amd import metrics
    img, gt = metrics_cases.pair("noise")
    H, W = img.shape[:2]
    m = metrics_cases.ssim_map_numpy(img, gt)
    sums = np.array([metrics_cases.sq_err_sum_numpy(img, gt), m.sum()])
    want_psnr = -10.0 * np.log10(np.mean(np.square(img - gt), dtype=np.float64))
    assert abs(metrics.psnr_from_sums(sums, H, W) - want_psnr) <= 1e-12
    assert abs(metrics.ssim_from_sums(sums, H, W) - m.mean()) <= 1e-14
    assert abs(metrics.mean_ssim(sums[1], H, W) - m.mean()) <= 1e-14
    t = torch.from_numpy(np.stack([sums, sums]))
    assert torch.allclose(metrics.psnr_from_sums(t, H, W), torch.full((2,), want_psnr, dtype=torch.float64), rtol=0, atol=1e-12)
    assert metrics.ssim_from_sums(t, H, W).shape == (2,)


def test_render_viewpoints_eval_ssim_argument_errors():
    """eval_ssim without ground truth, or with a render factor, is an error (the reference skips the metric silently); both are
    raised before the model is touched"""
    from unboundednerfpytorch_amd.run_render import render_viewpoints
    poses, HW, Ks = [np.eye(4, dtype=np.float32)], [(16, 16)], [np.eye(3)]
    gt = [np.zeros((16, 16, 3), np.float32)]
    with pytest.raises(ValueError, match="gt_imgs"):
        render_viewpoints(None, poses, HW, Ks, {"stepsize": 0.5}, eval_ssim=True)
    with pytest.raises(ValueError, match="render_factor"):
        render_viewpoints(None, poses, HW, Ks, {"stepsize": 0.5}, gt_imgs=gt, render_factor=2, eval_ssim=True)
    with pytest.raises(ValueError, match="gt_imgs\\[0\\]"):
        render_viewpoints(None, poses, HW, Ks, {"stepsize": 0.5}, gt_imgs=[np.zeros((16, 15, 3), np.float32)], eval_ssim=True)
    with pytest.raises(ValueError, match="11"):
        render_viewpoints(None, poses, [(10, 16)], Ks, {"stepsize": 0.5}, gt_imgs=[np.zeros((10, 16, 3), np.float32)], eval_ssim=True)


def test_install_metrics_rebinds_rgb_ssim():
    from unboundednerfpytorch_amd import compat, metrics
    old = lambda *a, **k: None
    utils = types.SimpleNamespace(rgb_ssim=old, other=1)
    assert compat.install_metrics(utils) is old
    assert utils.rgb_ssim is metrics.rgb_ssim and utils.other == 1
    mod = types.ModuleType("utils_standin")
    assert compat.install_metrics(mod) is None and mod.rgb_ssim is metrics.rgb_ssim


def test_metrics_kernels_keep_everything_in_registers(lib):
    """no VGPR / SGPR spills and no private segment in the two kernels of csrc/ugrid_metrics.hip; the main kernel runs one
    workgroup of four waves per CU (its 102 KB of LDS decide that), so it may use the whole 512-register file of a lane"""
    from test_capi import _kernel_metadata
    meta = _kernel_metadata(os.path.join(ROOT, "unboundednerfpytorch_amd", "libugrid_hip.so"))
    for prefix, limit in (("_Z15k_frame_metricsPK", 512), ("_Z19k_frame_metrics_sum", 64)):
        ks = [k for k in meta if k.startswith(prefix)]
        assert len(ks) == 1, (prefix, ks)
        m = meta[ks[0]]
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0 and m.get("private_segment_fixed_size", 0) == 0, (ks[0], m)
        assert m["vgpr_count"] <= limit, (ks[0], m)
