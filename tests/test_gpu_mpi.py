"""Forward-facing DirectMPIGO render on the GPU (mpi_render.DirectMPIGORenderer): the composed HIP path and the fused march
(ugrid_render_march_mpi) + shade kernels vs the reference's goldens, fused vs composed on an LLFF-shaped view, the NDC ray
kernel, the frame loop, the checkpoint route and the rgbnet arithmetic modes of the (0, 9, 0) shade instantiation."""
import os

import numpy as np
import pytest
import torch

import mpi_cases

pytestmark = pytest.mark.gpu


def _golden_rays(case):
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    return [torch.from_numpy(a).cuda() for a in mpi_cases.ndc_rays(seed, R)]


def _check_golden(out, gold):
    for k in ("alphainv_last", "rgb_marched", "depth"):
        np.testing.assert_allclose(out[k].cpu().numpy(), gold[k], rtol=0, atol=1e-4, err_msg=k)


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=[c[0] for c in mpi_cases.MPI_CASES])
def test_mpi_composed_hip_matches_reference_golden(case, golden_dir):
    """(a) the composed forward over the HIP drop-in ops"""
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    gold = np.load(os.path.join(golden_dir, case[0] + ".npz"))
    o, d, v = _golden_rays(case)
    out = DirectMPIGORenderer(mpi_cases.state(case), "cuda:0")(o, d, v, near=0, far=1, stepsize=case[5], bg=1, render_depth=True)
    assert abs(out["ray_id"].shape[0] - gold["ray_id"].shape[0]) <= 2
    _check_golden(out, gold)


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=[c[0] for c in mpi_cases.MPI_CASES])
def test_mpi_fused_matches_reference_golden(case, golden_dir):
    """(b) the fused march + shade kernels (C = 9 rgbnet of configs/llff, and the no-rgbnet model through the direct shade)"""
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    gold = np.load(os.path.join(golden_dir, case[0] + ".npz"))
    rend = DirectMPIGORenderer(mpi_cases.state(case), "cuda:0")
    assert rend.fused_supported()
    o, d, v = _golden_rays(case)
    out = rend.render_rays(o, d, v, near=0, far=1, stepsize=case[5], bg=1, render_depth=True)
    assert set(out) == {"rgb_marched", "depth", "alphainv_last"}
    _check_golden(out, gold)


_LLFF = {}


def llff_scene():
    """an LLFF-shaped model: mpi_depth 128, ~128^2 x 128 voxels, the llff_default C = 9 / width 64 / pe 0 rgbnet, white-noise grids"""
    if not _LLFF:
        from unboundednerfpytorch_amd.mpi_render import mpi_state_from_params
        D, nvox, C, stepsize = 128, 128 ** 3, 9, 0.5
        ws = mpi_cases.world_size(nvox, D)
        p = mpi_cases.mpi_params(51, ws, C, 0.0, 3.0)
        names = ['rgbnet.0', 'rgbnet.2.0', 'rgbnet.3']
        st = mpi_state_from_params(mpi_cases.XYZ_MIN, mpi_cases.XYZ_MAX, nvox, D, torch.from_numpy(p['density.grid']),
                                   torch.from_numpy(p['act_shift.grid']), torch.from_numpy(p['k0.grid']),
                                   [torch.from_numpy(p[n + '.weight']) for n in names], [torch.from_numpy(p[n + '.bias']) for n in names],
                                   torch.from_numpy(p['mask_cache.mask']), mpi_cases.fast_color_thres(stepsize, D), 0)
        _LLFF.update(state=st, world_size=ws, stepsize=stepsize)
    return _LLFF


def llff_view(H=304, W=400):
    K = np.array([[350.0, 0, W / 2], [0, 350.0, H / 2], [0, 0, 1]])
    ang = 0.05
    c2w = torch.tensor([[np.cos(ang), 0, np.sin(ang), 0.05], [0.0, 1.0, 0, -0.03], [-np.sin(ang), 0, np.cos(ang), 0.1]],
                       dtype=torch.float32)
    return H, W, K, c2w


def test_mpi_fused_vs_composed_llff_view():
    """(c) a 400 x 304 LLFF-shaped view (mpi_depth 128, stepsize 0.5, world_xy ~ 128) through the fused kernels vs the composed
    forward chunked like the reference, incl. rays that leave the box and a ray count that is not a multiple of 64"""
    from unboundednerfpytorch_amd.fourier_render import get_rays_of_a_view
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    sc = llff_scene()
    assert abs(sc["world_size"][0] - 128) < 8 and sc["world_size"][2] == 128
    rend = DirectMPIGORenderer(sc["state"], "cuda:0")
    assert rend.fused_supported()
    H, W, K, c2w = llff_view()
    o, d, v = [x.reshape(-1, 3).contiguous() for x in get_rays_of_a_view(H, W, K, c2w.cuda(), ndc=True)]
    o[:64, 0] += 1.5                 # origins beyond the box's x range: these rays enter it late or never
    d[64:128, 1] *= 3.0              # steep rays that leave it through the y faces
    n = H * W - 37
    o, d, v = o[:n].contiguous(), d[:n].contiguous(), v[:n].contiguous()
    kw = dict(near=0, far=1, stepsize=sc["stepsize"], bg=1, render_depth=True)
    got = rend.render_rays(o, d, v, ray_order="coherent", **kw)
    ref = {k: [] for k in ("rgb_marched", "depth", "alphainv_last")}
    for b in range(0, n, 8192):
        r = rend(o[b:b + 8192], d[b:b + 8192], v[b:b + 8192], **kw)
        for k in ref:
            ref[k].append(r[k])
    ref = {k: torch.cat(x) for k, x in ref.items()}
    assert float((ref["alphainv_last"] < 0.99).float().mean()) > 0.2
    thres = float(sc["state"]["fast_color_thres"])
    bad = torch.zeros(n, dtype=torch.bool, device="cuda")
    for k in ("rgb_marched", "alphainv_last", "depth"):
        e = (got[k] - ref[k]).abs()
        e = e.amax(dim=1) if e.dim() == 2 else e
        bad |= e > 1e-4
        # a threshold flip moves a pixel by at most about the weight threshold (7.8e-4 here: stepsize / mpi_depth / 5); depth < 1
        assert float(e.max()) < 2 * thres, (k, float(e.max()))
    assert int(bad.sum()) <= max(2, n // 20000), int(bad.sum())
    assert torch.isfinite(got["rgb_marched"]).all()
    miss = ref["alphainv_last"] == 1
    assert int(miss[:128].sum()) > 0 and torch.equal(got["alphainv_last"][miss], ref["alphainv_last"][miss])


def test_ndc_ray_kernel_matches_reference(golden_dir):
    """(d) ugrid_rays_of_a_view_ndc == dvgo.get_rays_of_a_view(ndc=True), whole view and a pixel-index list"""
    from unboundednerfpytorch_amd.fourier_render import get_rays_of_a_view, get_rays_of_pixel_index
    g = np.load(os.path.join(golden_dir, "rays_view_ndc.npz"))
    c2w = torch.from_numpy(g["c2w"]).cuda()
    perm = torch.randperm(48, generator=torch.Generator().manual_seed(0)).cuda()
    for tag, kw in (("a", dict(inverse_y=False, flip_x=False, flip_y=False)),
                    ("b", dict(inverse_y=True, flip_x=True, flip_y=False)),
                    ("c", dict(inverse_y=False, flip_x=False, flip_y=True))):
        o, d, v = get_rays_of_a_view(6, 8, g["K"], c2w, ndc=True, **kw)
        po, pd, pv = get_rays_of_pixel_index(6, 8, g["K"], c2w, perm, ndc=True, **kw)
        for a, pa, k in ((o, po, "_o"), (d, pd, "_d"), (v, pv, "_v")):
            want = g[tag + k]
            np.testing.assert_allclose(a.cpu().numpy(), want, rtol=1e-6, atol=1e-7, err_msg=tag + k)
            assert torch.equal(pa, a.reshape(-1, 3)[perm]), tag + k


def test_mpi_render_viewpoints_frames_in_flight():
    """(e) run_render.render_viewpoints drives the renderer unchanged; 3 views, bit-identical frames at 1 and 2 in flight"""
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
    one = render_viewpoints(rend, poses, [(H, W)] * 3, [K] * 3, kw, frames_in_flight=1)
    two = render_viewpoints(rend, poses, [(H, W)] * 3, [K] * 3, kw, frames_in_flight=2)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    view = rend.render_view(H, W, K, torch.from_numpy(poses[1]), render_depth=True, **kw)
    assert np.array_equal(view["rgb_marched"].cpu().numpy(), one[0][1])
    assert float(one[2].mean()) < 0.95 and np.isfinite(one[0]).all()


def test_mpi_checkpoint_to_golden(golden_dir):
    """(f) the reference's checkpoint of the mpi_fine model -> DirectMPIGORenderer -> the reference's outputs"""
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    ckpt = torch.load(os.path.join(golden_dir, "mpi_ckpt_small.tar"), map_location="cpu", weights_only=False)
    rend = DirectMPIGORenderer.from_reference_checkpoint(ckpt, "cuda:0")
    assert rend.fused_supported()
    case = mpi_cases.MPI_CASES[0]
    o, d, v = _golden_rays(case)
    _check_golden(rend.render_rays(o, d, v, near=0, far=1, stepsize=case[5], bg=1, render_depth=True),
                  np.load(os.path.join(golden_dir, "mpi_fine.npz")))


def test_mpi_shade_triple_is_instantiated():
    """(g) configs/llff's net (rgbnet_dim 9, viewbase_pe 0) on single-level k0"""
    from unboundednerfpytorch_amd import _lib
    assert _lib.load().ugrid_shade_supported(0, 9, 0) == 1


def test_mpi_fused_frame_in_all_mlp_modes():
    """(h) fp32 / bf16x3 / fp16x2 rgbnet arithmetic of the (0, 9, 0) shade kernels give the same frame"""
    from unboundednerfpytorch_amd import _lib
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    sc = llff_scene()
    H, W, K, c2w = llff_view(96, 128)
    frames = {}
    for mode in (_lib.MLP_FP32, _lib.MLP_BF16X3, _lib.MLP_FP16X2):
        rend = DirectMPIGORenderer(sc["state"], "cuda:0", mlp_mode=mode)
        out = rend.render_view(H, W, K, c2w, near=0, far=1, stepsize=sc["stepsize"], bg=1, render_depth=True)
        assert rend._fused_renderer().mlp_mode == mode
        frames[mode] = out["rgb_marched"]
    for mode in (_lib.MLP_BF16X3, _lib.MLP_FP16X2):
        assert float((frames[mode] - frames[_lib.MLP_FP32]).abs().max()) < 1e-5, mode
    assert float(frames[_lib.MLP_FP32].std()) > 1e-3
