"""The coarse stage (no rgbnet, 3-channel k0) on the native step, and the fused stage set-up -- HOST side, on the CPU: which
configurations select native_step.VoxGOStep with colour 'none' (opt-in: TrainModel.native_coarse), the struct mirror with the
renamed `colour` field, the workspaces of colour 1, and the dispatch of train_rays.voxel_count_views / hit_coarse_geo (CPU
tensors keep the composed paths).  The kernels' results are tests/test_gpu_coarse_native.py's and tests/test_gpu_stage_setup.py's
business."""
import ctypes

import numpy as np
import pytest
import torch

import synth
from test_mpi_native_host import model as mpi_model

KW = dict(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=12 ** 3, num_voxels_base=12 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
FG = dict(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels_density=10 ** 3, num_voxels_base_density=10 ** 3, num_voxels_rgb=10 ** 3,
          num_voxels_base_rgb=10 ** 3, num_voxels_viewdir=-1, alpha_init=1e-4, fast_color_thres=1e-4, fourier_freq_num=2)


def _coarse_models():
    from unboundednerfpytorch_amd import voxgo_model as vm
    return [vm.DirectVoxGO(rgbnet_dim=0, **KW), vm.DirectContractedVoxGO(rgbnet_dim=0, **KW)]


def test_the_coarse_stage_takes_the_native_step_only_when_asked():
    for m in _coarse_models():
        assert m.native_coarse is False and m.rgbnet is None
        assert m._native_params() is None                         # the default: the op-by-op ops
        m.native_coarse = True
        p = m._native_params()
        assert p is not None and len(p) == 8
        assert p[0] is m.density.grid and p[1] is m.k0.grid and p[1].shape[1] == 3
        assert p[2:] == [None] * 6
        # still not the native step's business: a frozen grid, no gradient, native_step off
        for g in (m.density.grid, m.k0.grid):
            g.requires_grad_(False)
            assert m._native_params() is None
            g.requires_grad_(True)
        with torch.no_grad():
            assert m._native_params() is None
        assert m._native_params() is not None
        m.native_step = False
        assert m._native_params() is None


def test_native_coarse_leaves_the_fine_stage_and_the_other_models_alone():
    from unboundednerfpytorch_amd import voxgo_model as vm
    from unboundednerfpytorch_amd.fourier_model import FourierGridModel
    fine = vm.DirectVoxGO(rgbnet_dim=12, rgbnet_direct=True, **KW)
    before = fine._native_params()
    fine.native_coarse = True
    after = fine._native_params()
    assert len(before) == len(after) == 8 and all(a is b for a, b in zip(before, after))
    mpi = mpi_model(rgbnet_dim=0)
    assert mpi.rgbnet is None and mpi._native_params() is None
    mpi.native_coarse = True
    assert mpi._native_params() is None                          # DirectMPIGO ignores the attribute
    fg = FourierGridModel(rgbnet_dim=0, **FG)
    assert fg.rgbnet is None
    fg.native_coarse = True
    assert fg._native_params() is None                           # FourierGridModel too


def test_colour_field_keeps_the_struct_and_shrinks_the_workspaces():
    from unboundednerfpytorch_amd import _lib
    lib = _lib.load()
    assert ctypes.sizeof(_lib.VoxgoStep) == lib.ugrid_voxgo_step_sizeof()
    names = [n for n, _ in _lib.VoxgoStep._fields_]
    assert "colour" in names and "reserved_" not in names
    assert names[names.index("colour") - 1] == "sync_free" and names[names.index("colour") + 1] == "ws"
    assert _lib.VoxgoStep.colour.offset == _lib.VoxgoStep.sync_free.offset + 4 and _lib.VoxgoStep.colour.size == 4
    assert lib.ugrid_abi_version() == 3

    def step(colour, C, pe, width):
        s = _lib.VoxgoStep()
        s.mode, s.P, s.kP, s.slots = 0, 1, 1, 40
        s.colour, s.C, s.pe, s.width, s.n_rays, s.M1, s.M2 = colour, C, pe, width, 8192, 1000, 130
        return s
    al = lambda n: (n + 63) & ~63
    net, none = step(0, 3, 4, 128), step(1, 3, 0, 0)
    fw = [lib.ugrid_voxgo_step_ws_floats(ctypes.addressof(s)) for s in (net, none)]
    bw = [lib.ugrid_voxgo_step_bwd_ws_floats(ctypes.addressof(s)) for s in (net, none)]
    assert fw[1] < fw[0] and bw[1] < bw[0]
    # colour 1: the sampling's arrays and the loss's gradients only -- nothing for k0, feat, h1, h2, ray_rows, g_k0 or the rgbnet scratch
    assert fw[1] == al(3000) + 4 * al(1000) + al(390)
    assert bw[1] == al(390) + 2 * al(130) + al(8192) + al(1000)
    # entry points refuse, before touching the device: another colour value, colour 1 on a k0 that is not 3 channels
    for bad in (step(2, 3, 0, 0), step(-1, 3, 0, 0), step(1, 12, 0, 0)):
        assert lib.ugrid_voxgo_step_forward(ctypes.addressof(bad), None) == 1          # hipErrorInvalidValue


def test_voxgo_step_refuses_weights_with_colour_none_before_any_launch():
    from unboundednerfpytorch_amd import native_step
    m = _coarse_models()[0]
    w = torch.zeros(3, 3)
    with pytest.raises(RuntimeError, match="colour 'none'"):
        native_step.VoxGOStep.apply(m.density.grid, m.k0.grid, w, None, None, None, None, None,
                                    {'colour': 'none', 'mode': 'dvgo', 'cfg': {}, 'rays_o': torch.zeros(2, 3), 'rays_d': torch.ones(2, 3),
                                     'target': torch.zeros(2, 3)})


def test_set_up_utilities_keep_the_composed_path_on_cpu_tensors(monkeypatch):
    """CPU rays (the oracle back-end of tests/test_dvgo.py, a host-resident ray table) never reach the fused kernels: the entry
    points are replaced by ones that fail, the composed paths run over stand-in ops and give their results"""
    from unboundednerfpytorch_amd import _lib, train_rays
    from unboundednerfpytorch_amd import render_utils_cuda as own
    assert train_rays.FUSED_SETUP is True

    class Trap:
        def __getattr__(self, name):
            raise AssertionError("fused entry point %s reached with CPU tensors" % name)
    monkeypatch.setattr(_lib, "load", lambda: Trap())
    monkeypatch.setattr(train_rays, "voxel_count_views_fused", lambda *a, **k: (_ for _ in ()).throw(AssertionError("fused")))
    lo, hi = torch.zeros(3), torch.full((3,), 4.0)
    ws = torch.tensor([5, 5, 5])
    o = torch.tensor([[2.0, 2.0, -1.0], [1.0, 3.0, -1.0]])
    d = torch.tensor([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]])
    seen = []

    class Query(torch.autograd.Function):              # a differentiable stand-in lookup: every point adds 0.75 to voxel 0
        @staticmethod
        def forward(ctx, grid, pts, lo_, hi_, F):
            ctx.n, ctx.shape = pts[..., 0].numel(), grid.shape
            seen.append(tuple(pts.shape))
            return pts.new_zeros(pts.shape[:-1])

        @staticmethod
        def backward(ctx, g):
            out = torch.zeros(ctx.shape)
            out.view(-1)[0] = 0.75 * ctx.n
            return out, None, None, None, None
    count = train_rays.voxel_count_views(Query.apply, lo, hi, torch.tensor(1.0), ws, (1, 1, 5, 5, 5), o, d, [1, 1], 0.2, 0.5,
                                         irregular_shape=True)
    n_samples = int(np.linalg.norm(np.array([6.0, 6.0, 6.0])) / 0.5) + 1
    assert seen == [(1, n_samples, 3)] * 2 and float(count.sum()) == 2.0 and float(count.view(-1)[0]) == 2.0

    calls = []

    def sample_pts_on_rays(o_, d_, lo_, hi_, near, far, stepdist):
        calls.append("sample")
        pts = torch.zeros(3, 3)
        return [pts, torch.tensor([False, True, False]), torch.tensor([0, 0, 1]), None]

    def maskcache_lookup(mask, pts, scale, shift):
        calls.append("lookup")
        return torch.tensor([False, True])
    # the package's own module, but CPU rays: composed
    monkeypatch.setattr(own, "sample_pts_on_rays", sample_pts_on_rays)
    monkeypatch.setattr(own, "maskcache_lookup", maskcache_lookup)
    hit = train_rays.hit_coarse_geo(own, o, d, lo, hi, 0.2, 0.5, torch.ones(5, 5, 5, dtype=torch.bool), torch.ones(3), torch.zeros(3))
    assert calls == ["sample", "lookup"] and hit.tolist() == [False, True]
