"""Frame metrics on the GPU (unboundednerfpytorch_amd.metrics -> ugrid_frame_metrics, csrc/ugrid_metrics.hip) against the
reference's own SSIM maps (tests/golden/ssim_maps.npz, written by tests/golden/gen_golden_metrics.py) on the seeded image pairs
of tests/metrics_cases.py, and the frame loop's eval_ssim.

Bar of the map: 1e-9 absolute on every element and on the mean.  Both sides do the same fp64 operations on the same fp32 inputs
and differ in the order (and, in the kernel, the fusing) of the 2 x 11 additions of a blur: <= 22 roundings of 2.2e-16 on values
up to 1, amplified by at most 1 / c2 = 1.1e3 in the quotient -- of order 1e-11; the bar leaves two orders of margin."""
import os

import numpy as np
import pytest
import torch

import metrics_cases
import mpi_cases

pytestmark = pytest.mark.gpu

NAMES = list(metrics_cases.PAIRS)


@pytest.fixture(scope="module")
def golden_maps(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ssim_maps.npz")))


def _dev(a):
    return torch.from_numpy(a).cuda()


@pytest.mark.parametrize("name", NAMES)
def test_map_and_mean_match_the_reference(name, golden_maps):
    from unboundednerfpytorch_amd import metrics
    img, gt = metrics_cases.pair(name)
    H, W = img.shape[:2]
    gold = golden_maps[name]
    sums, m = metrics.frame_metrics(_dev(img), _dev(gt), max_val=1.0, return_map=True)
    assert sums.dtype == torch.float64 and sums.shape == (2,) and m.dtype == torch.float64 and tuple(m.shape) == gold.shape
    m = m.cpu().numpy()
    sums = sums.cpu().numpy()
    mean = metrics.mean_ssim(sums[1], H, W)
    d_map, d_mean = float(np.abs(m - gold).max()), abs(mean - float(gold.mean()))
    print("%s: %d x %d  max |map - reference| = %.3e  |mean - reference| = %.3e" % (name, H, W, d_map, d_mean))
    assert np.isfinite(m).all()
    assert d_map <= 1e-9
    assert d_mean <= 1e-9
    if name == "identical":
        assert (m == 1.0).all() and sums[0] == 0.0
    # the sums without the map take the same path
    assert torch.equal(metrics.frame_metrics(_dev(img), _dev(gt)).cpu(), torch.from_numpy(sums))


@pytest.mark.parametrize("name", NAMES)
def test_squared_error_sum_matches_numpy(name):
    from unboundednerfpytorch_amd import metrics
    img, gt = metrics_cases.pair(name)
    want = metrics_cases.sq_err_sum_numpy(img, gt)
    got = float(metrics.frame_metrics(_dev(img), _dev(gt))[0].item())
    print("%s: sum of squares %.17g (numpy %.17g)" % (name, got, want))
    assert abs(got - want) <= 1e-12 * abs(want)
    H, W = img.shape[:2]
    if want > 0:
        psnr = float(metrics.psnr_from_sums(metrics.frame_metrics(_dev(img), _dev(gt)), H, W).item())
        assert abs(psnr - (-10.0 * np.log10(want / (H * W * 3)))) <= 1e-10


@pytest.mark.parametrize("name", ["thin_ragged", "tile_2p3_m1", "flat_bright"])
def test_pixel_stride_does_not_change_the_bits(name):
    """[H*W,3] rows and the rgb columns of [H*W,5] rows (the frame loop's packed layout, read in place) give equal results"""
    from unboundednerfpytorch_amd import metrics
    img, gt = metrics_cases.pair(name)
    H, W = img.shape[:2]
    a3, g3 = _dev(img).reshape(-1, 3), _dev(gt).reshape(-1, 3)
    a5 = torch.full((H * W, 5), float("nan"), device="cuda")
    a5[:, :3] = a3
    s3, m3 = metrics.frame_metrics(a3, g3, H=H, W=W, return_map=True)
    s5, m5 = metrics.frame_metrics(a5, g3, H=H, W=W, return_map=True)
    s5b = metrics.frame_metrics(a5[:, :3], g3, H=H, W=W)
    sv = metrics.frame_metrics(_dev(img), _dev(gt))
    assert torch.equal(s3, s5) and torch.equal(m3, m5) and torch.equal(s3, s5b) and torch.equal(s3, sv)
    out = torch.zeros(4, 2, dtype=torch.float64, device="cuda")
    ws = torch.empty(metrics.workspace_bytes(H, W), dtype=torch.uint8, device="cuda")
    assert metrics.frame_metrics(a5, g3, H=H, W=W, out=out[2], ws=ws) is not None
    assert torch.equal(out[2], s3) and float(out[[0, 1, 3]].abs().sum()) == 0.0


@pytest.mark.parametrize("name", ["tile_m1_2p3", "negated"])
def test_two_calls_give_the_same_bits(name):
    from unboundednerfpytorch_amd import metrics
    img, gt = metrics_cases.pair(name)
    a, g = _dev(img), _dev(gt)
    s1, m1 = metrics.frame_metrics(a, g, return_map=True)
    s2, m2 = metrics.frame_metrics(a, g, return_map=True)
    assert torch.equal(s1, s2) and torch.equal(m1, m2)


def test_argument_errors_on_device_tensors():
    from unboundednerfpytorch_amd import metrics
    a = torch.zeros(16, 16, 3, device="cuda")
    with pytest.raises(ValueError):
        metrics.frame_metrics(a[:10], a[:10])
    with pytest.raises(ValueError):
        metrics.frame_metrics(a[:, :10].contiguous(), a[:, :10].contiguous())
    with pytest.raises(ValueError):
        metrics.frame_metrics(a, torch.zeros(16, 17, 3, device="cuda"))
    with pytest.raises(ValueError):
        metrics.frame_metrics(a, a, filter_size=9)


def test_reference_signature_wrapper(golden_maps):
    """metrics.rgb_ssim on numpy input: a Python float, or the fp64 numpy map; float64 input is rounded to float32"""
    from unboundednerfpytorch_amd import metrics
    img, gt = metrics_cases.pair("noise")
    gold = golden_maps["noise"]
    v = metrics.rgb_ssim(img, gt, 1)
    assert type(v) is float and abs(v - float(gold.mean())) <= 1e-9
    m = metrics.rgb_ssim(img, gt, 1, return_map=True)
    assert isinstance(m, np.ndarray) and m.dtype == np.float64 and m.shape == gold.shape and np.abs(m - gold).max() <= 1e-9
    assert metrics.rgb_ssim(img.astype(np.float64), gt.astype(np.float64), max_val=1) == v
    assert metrics.rgb_ssim(torch.from_numpy(img), _dev(gt), 1.0) == v
    # the other runtime arguments reach the kernel
    want = metrics_cases.ssim_map_numpy(img, gt, max_val=2.0, filter_sigma=2.0, k1=0.02, k2=0.05)
    got = metrics.rgb_ssim(img, gt, 2.0, 11, 2.0, 0.02, 0.05, True)
    assert np.abs(got - want).max() <= 1e-9


def test_frame_loop_eval_ssim():
    """render_viewpoints(eval_ssim=True): five items, the first four those of the call without it, ssims the same at 1 and 2 frames
    in flight, equal to metrics.rgb_ssim on the returned frames exactly and to the numpy formula to 1e-9"""
    from unboundednerfpytorch_amd import metrics
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    from unboundednerfpytorch_amd.run_render import render_viewpoints
    case = mpi_cases.MPI_CASES[0]
    rend = DirectMPIGORenderer(mpi_cases.state(case), "cuda:0")
    H, W = 48, 64
    K = np.array([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]])
    poses = []
    for a in (-0.05, 0.0, 0.04):
        poses.append(np.array([[np.cos(a), 0, np.sin(a), 0.1 * a], [0, 1, 0, 0.02], [-np.sin(a), 0, np.cos(a), 0.05], [0, 0, 0, 1]],
                              dtype=np.float32))
    kw = dict(near=0, far=1, stepsize=case[5], bg=1)
    args = (rend, poses, [(H, W)] * 3, [K] * 3, kw)
    plain = render_viewpoints(*args)
    rs = np.random.RandomState(7)
    gt = [np.clip(plain[0][i] + 0.05 * rs.randn(H, W, 3), 0.0, 1.0).astype(np.float32) for i in range(3)]
    base = render_viewpoints(*args, gt_imgs=gt)
    assert len(base) == 4
    one = render_viewpoints(*args, gt_imgs=gt, eval_ssim=True, frames_in_flight=1)
    two = render_viewpoints(*args, gt_imgs=gt, eval_ssim=True, frames_in_flight=2)
    for res in (one, two):
        assert len(res) == 5
        for a, b in zip(res[:4], base):
            assert np.array_equal(np.asarray(a), np.asarray(b))
        for a, b in zip(res[:3], plain):
            assert np.array_equal(a, b)
    assert one[4] == two[4] and len(one[4]) == 3 and all(type(v) is float for v in one[4])
    for i in range(3):
        assert one[4][i] == metrics.rgb_ssim(one[0][i], gt[i], max_val=1)
        want = float(metrics_cases.ssim_map_numpy(one[0][i], gt[i]).mean())
        print("view %d: ssim %.12f  |device - numpy| = %.3e" % (i, one[4][i], abs(one[4][i] - want)))
        assert abs(one[4][i] - want) <= 1e-9
        assert 0.0 < one[4][i] < 1.0
    # float64 ground truth (what np.clip of a float64 sum hands over) is rounded to float32 on upload
    gt64 = [g.astype(np.float64) for g in gt]
    assert render_viewpoints(*args, gt_imgs=gt64, eval_ssim=True)[4] == one[4]
