"""TensoRF grids, the CPU half: the float64 formula of tests/tensorf_cases.py against the reference's own float64 module (fixture),
the exact-bake argument in float64, and the host side of grid.TensoRFGrid / the two VoxGO models (construction, state dict,
get_kwargs, checkpoints, the path a TensoRF model takes).  The kernels themselves: tests/test_gpu_tensorf.py."""
import os

import numpy as np
import pytest
import torch

import tensorf_cases as tc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {c[0]: c for c in tc.KERNEL_CASES}


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLD, "tensorf_kernels.npz"))


def test_recorded_yardsticks_are_tight():
    """the bound 4 x yardstick cannot become vacuous: every recorded fp32-vs-fp64 error of the reference -- for every case and every
    point count -- is below 1e-5 of its tensor's largest magnitude"""
    y = tc.load_yardsticks(GOLD)
    assert sorted(y) == sorted(CASES)
    for name, case in CASES.items():
        for n in tc.N_POINTS:
            seen = 0
            for key, (err, scale) in y[name].items():
                if key.startswith("n%d/" % n):
                    assert err <= 1e-5 * scale, (name, key, err, scale)
                    assert n == 0 or key.split("/")[1].startswith("tv_") or n < max(tc.N_POINTS) or (scale > 0 and err > 0), (name, key)
                    seen += 1
            full = n == max(tc.N_POINTS)          # (the TV gradient and the dense grid do not depend on the points: recorded once)
            assert seen == 1 + 6 + (1 if case[5] > 1 else 0) + (7 if full else 0), (name, n, seen)


@pytest.mark.parametrize("name", [c for c in CASES if not c.startswith("path_")])
def test_fp64_formula_is_the_reference_in_float64(fixture, name):
    n = max(tc.N_POINTS)
    mine = tc.reference_f64(CASES[name], n)
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-3)
    assert close(mine['out'][:tc.N_STORED], fixture[name + "/out64"])
    keys = [str(k) for k in fixture[name + "/keys"]]
    assert keys == list(tc.shapes(*CASES[name][2:]))           # the reference's parameter names, in its order
    for k in keys:
        assert close(mine['g_' + k], fixture["%s/g_%s/64" % (name, k)]), k
        assert fixture["%s/g_%s/64" % (name, k)].shape == tc.shapes(*CASES[name][2:])[k]
    for k in tc.FACTORS:
        assert close(mine['tv_' + k], fixture["%s/tv_%s/64" % (name, k)]), k


@pytest.mark.parametrize("name", list(CASES))
def test_bake_then_trilinear_is_the_factorised_query_in_float64(name):
    """trilinear weights are separable, so trilinear interpolation of the dense grid sum_r plane_r[i,j] vec_r[k] equals the
    factorised interpolation term by term -- out-of-box points (zero padding) included"""
    params, pts, _ = tc.case_inputs(CASES[name])
    p = tc.as_f64(params)
    q = tc.query(p, torch.from_numpy(pts))
    t = tc.trilinear(tc.dense(p), torch.from_numpy(pts))
    t = t[:, 0] if q.dim() == 1 else t
    assert float((q - t).abs().max()) <= 1e-12 * max(float(q.abs().max()), 1e-3)
    outside = ((pts < np.float32(tc.XYZ_MIN)) | (pts > np.float32(tc.XYZ_MAX))).any(1)
    assert outside.sum() > 1000 and float(q[torch.from_numpy(outside)].abs().max()) > 0


def test_create_grid_dispatch_shapes_and_initial_statistics():
    from unboundednerfpytorch_amd import grid
    ws = torch.tensor([20, 30, 40])
    torch.manual_seed(0)
    g = grid.create_grid('TensoRFGrid', channels=12, world_size=ws, xyz_min=tc.XYZ_MIN, xyz_max=tc.XYZ_MAX, config={'n_comp': 24, 'n_comp_xy': 16},
                         component_last=True)
    assert isinstance(g, grid.TensoRFGrid)
    want = tc.shapes((20, 30, 40), 24, 16, 12)
    assert {k: tuple(v.shape) for k, v in g.state_dict().items() if k not in ('xyz_min', 'xyz_max')} == want
    assert list(g.state_dict()) == list(want) + ['xyz_min', 'xyz_max']          # (parameters, then buffers: the reference's order)
    for k in tc.FACTORS:                     # N(0, 0.1); component_last = True: stored component-last
        v = getattr(g, k)
        assert abs(float(v.detach().mean())) < 0.02 and abs(float(v.detach().std()) - 0.1) < 0.02, k
        assert v.is_contiguous(memory_format=torch.channels_last) and not v.is_contiguous()
    bound = 1 / np.sqrt(12)                  # kaiming_uniform_(a = sqrt(5)) of a [64, 12] tensor: U(-1/sqrt(fan_in), 1/sqrt(fan_in)), fan_in = 12
    assert float(g.f_vec.abs().max()) <= bound and float(g.f_vec.abs().max()) > 0.9 * bound
    assert g.extra_repr() == 'channels=12, world_size=[20, 30, 40], n_comp=24'
    # the same generator state gives the reference's own draws (same order of the same calls)
    torch.manual_seed(0)
    xy = torch.randn([1, 16, 20, 30]) * 0.1
    assert torch.equal(g.xy_plane.detach().contiguous(), xy)
    g1 = grid.create_grid('TensoRFGrid', channels=1, world_size=ws, xyz_min=tc.XYZ_MIN, xyz_max=tc.XYZ_MAX, config={'n_comp': 8})
    assert not hasattr(g1, 'f_vec') and g1.z_vec.shape == (1, 8, 40, 1) and g1.xy_plane.is_contiguous()      # the default: canonical
    d = grid.create_grid('DenseGrid', channels=3, world_size=ws, xyz_min=tc.XYZ_MIN, xyz_max=tc.XYZ_MAX, config={})
    assert isinstance(d, grid.FourierGrid) and d.grid.shape == (1, 3, 20, 30, 40)
    with pytest.raises(NotImplementedError):
        grid.create_grid('HashGrid', channels=1, world_size=ws, xyz_min=tc.XYZ_MIN, xyz_max=tc.XYZ_MAX, config={})
    # scale_volume_grid: six bilinear resamplings, the layout kept
    g.scale_volume_grid(torch.tensor([25, 35, 45]))
    assert g.xz_plane.shape == (1, 24, 25, 45) and g.y_vec.shape == (1, 24, 35, 1) and g.xz_plane.is_contiguous(memory_format=torch.channels_last)


def test_query_hook_runs_the_torch_composition_on_the_cpu():
    """TensoRFGrid.query_fn = grid.tensorf_compose (six grid_sample calls, cat, mm): the CPU stand-in equals the float64 formula to
    fp32 rounding, forward and gradients"""
    from unboundednerfpytorch_amd import grid
    case = CASES["w579_r4_2_c3"]
    params, pts, go = tc.case_inputs(case)
    g = grid.TensoRFGrid(channels=3, world_size=torch.tensor(case[2]), xyz_min=tc.XYZ_MIN, xyz_max=tc.XYZ_MAX, config={'n_comp': 4, 'n_comp_xy': 2})
    g.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=False)
    g.query_fn = grid.tensorf_compose
    out = g(torch.from_numpy(pts))
    (out * torch.from_numpy(go)).sum().backward()
    want = tc.reference_f64(case, max(tc.N_POINTS))
    assert np.abs(out.detach().numpy() - want['out']).max() < 1e-5 * np.abs(want['out']).max()
    for k, v in g.named_parameters():
        assert v.grad.stride() == v.stride()
        assert np.abs(v.grad.numpy() - want['g_' + k]).max() < 1e-5 * np.abs(want['g_' + k]).max(), k


TENSORF_KW = dict(density_type='TensoRFGrid', density_config=dict(n_comp=8), k0_type='TensoRFGrid', k0_config=dict(n_comp=24))


def small_dvgo(**kw):
    from unboundednerfpytorch_amd.voxgo_model import DirectVoxGO
    args = dict(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=12 ** 3, num_voxels_base=12 ** 3, alpha_init=1e-2, fast_color_thres=1e-4,
                rgbnet_dim=12, rgbnet_direct=True, rgbnet_width=32, **TENSORF_KW)
    args.update(kw)
    return DirectVoxGO(**args)


def test_models_accept_tensorf_grids_and_take_the_composed_path():
    from unboundednerfpytorch_amd import grid
    from unboundednerfpytorch_amd.voxgo_model import DirectContractedVoxGO
    from unboundednerfpytorch_amd.mpi_model import DirectMPIGO
    m = small_dvgo()
    assert isinstance(m.density, grid.TensoRFGrid) and isinstance(m.k0, grid.TensoRFGrid)
    assert m.density.xy_plane.shape == (1, 8, 12, 12) and m.k0.f_vec.shape == (72, 12)
    keys = list(m.state_dict())
    for g, has_f in (('density', False), ('k0', True)):
        for k in ('xyz_min', 'xyz_max') + tc.FACTORS + (('f_vec',) if has_f else ()):
            assert g + '.' + k in keys
    assert not any(k.endswith('.grid') for k in keys)
    fake = torch.zeros(4, 3)
    fake_cuda = type('T', (), {'is_cuda': True})()
    assert m._can_fuse(fake) is False and m._can_fuse(fake_cuda) is False and m._native_params() is None
    mixed = small_dvgo(density_type='DenseGrid', density_config={})
    assert isinstance(mixed.density, grid.FourierGrid) and isinstance(mixed.k0, grid.TensoRFGrid)
    assert mixed._can_fuse(fake_cuda) is False and mixed._native_params() is None
    dense = small_dvgo(density_type='DenseGrid', density_config={}, k0_type='DenseGrid', k0_config={})
    assert dense._can_fuse(fake_cuda) is True                           # two dense grids: the path they took before
    assert m._density_grid_shape() == torch.Size([1, 1, 12, 12, 12]) == dense._density_grid_shape()
    with pytest.raises(NotImplementedError, match="TensoRFGrid density"):
        m.maskout_near_cam_vox(torch.zeros(1, 3), 0.1)
    c = DirectContractedVoxGO(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=12 ** 3, num_voxels_base=12 ** 3, alpha_init=1e-2,
                              fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_width=32, **TENSORF_KW)
    assert isinstance(c.k0, grid.TensoRFGrid) and c._can_fuse(fake_cuda) is False and c._native_params() is None
    assert c._density_grid_shape() == torch.Size([1, 1] + c.world_size.tolist())
    with pytest.raises(NotImplementedError):
        small_dvgo(k0_type='HashGrid')
    with pytest.raises(NotImplementedError):
        DirectMPIGO(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=4000, mpi_depth=16, **TENSORF_KW)


@pytest.mark.parametrize("case", tc.MODEL_CASES, ids=[c[0] for c in tc.MODEL_CASES])
def test_state_dict_keys_and_shapes_are_the_reference_models(case):
    """tests/golden/tensorf_models.npz holds the state dict of the REFERENCE's model: same names, same order, same shapes, and it loads"""
    from unboundednerfpytorch_amd.voxgo_model import DirectContractedVoxGO, DirectVoxGO
    name, kind, density_type, seed, _ = case
    z = np.load(os.path.join(GOLD, "tensorf_models.npz"))
    ref = {k[len(name) + 4:]: z[k] for k in z.files if k.startswith(name + "/sd/")}
    m = (DirectVoxGO if kind == 'dvgo' else DirectContractedVoxGO)(**tc.model_kwargs(kind, density_type))
    mine = m.state_dict()
    assert list(mine) == list(ref)
    assert {k: tuple(v.shape) for k, v in mine.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in ref.items()}, strict=True)


def test_get_kwargs_round_trip_and_checkpoint(tmp_path, monkeypatch):
    from unboundednerfpytorch_amd import grid, train_utils
    monkeypatch.setattr(grid.TensoRFGrid, 'component_last', True)        # the storage layout must not reach the file
    from unboundednerfpytorch_amd.voxgo_model import DirectVoxGO
    torch.manual_seed(1)
    m = small_dvgo()
    kw = m.get_kwargs()
    assert kw['density_type'] == kw['k0_type'] == 'TensoRFGrid' and kw['density_config'] == {'n_comp': 8} and kw['k0_config'] == {'n_comp': 24}
    m2 = DirectVoxGO(**kw)
    assert {k: tuple(v.shape) for k, v in m2.state_dict().items()} == {k: tuple(v.shape) for k, v in m.state_dict().items()}
    opt = train_utils.create_optimizer_or_freeze_model(m, {'lrate_density': 0.02, 'lrate_k0': 0.02, 'lrate_rgbnet': 1e-3, 'lrate_decay': 20,
                                                           'skip_zero_grad_fields': ['density', 'k0']}, 0)
    # one group per field, in the config's order: all six density factors; the six k0 factors + f_vec; the rgbnet
    assert [(len(g['params']), g['lr'], g['skip_zero_grad']) for g in opt.param_groups] == [(6, 0.02, True), (7, 0.02, True), (6, 1e-3, False)]
    path = str(tmp_path / "tensorf.tar")
    train_utils.save_checkpoint(path, m, opt, 7)
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert all(v.is_contiguous() for v in ck['model_state_dict'].values())      # the reference's row-major layout on disk
    m3, _ = train_utils.load_model(path, DirectVoxGO)
    for k, v in m.state_dict().items():
        assert torch.equal(m3.state_dict()[k], v), k
    assert m3.k0.xy_plane.is_contiguous(memory_format=torch.channels_last) and not m3.k0.xy_plane.is_contiguous()


def test_renderers_existing_entry_points_still_refuse_and_the_memory_guard_names_both_numbers():
    from unboundednerfpytorch_amd import bounded_render, dcvgo_render, dvgo_render
    m = small_dvgo()
    ck = {'model_kwargs': m.get_kwargs(), 'model_state_dict': m.state_dict()}
    with pytest.raises(NotImplementedError):
        dvgo_render.dvgo_state_from_reference_checkpoint(ck)
    with pytest.raises(NotImplementedError):
        dcvgo_render.dcvgo_state_from_reference_checkpoint(ck)
    need = 4 * (1 + 12) * 12 ** 3
    with pytest.raises(RuntimeError, match="needs %d bytes .* 1000 bytes are free" % need):
        bounded_render.bake_tensorf_checkpoint(ck, "cuda:0", mem_get_info=lambda dev: (1000, 2000))
    # the trainer's buffers win over what model_kwargs re-derives
    st = bounded_render.stored_buffers_win({'act_shift': torch.tensor([0.0]), 'other': 1}, {'model_state_dict': {'act_shift': torch.tensor([-5.5])}},
                                           ('act_shift', 'scene_radius'))
    assert float(st['act_shift']) == -5.5 and st['other'] == 1 and 'scene_radius' not in st


def _reference_available():
    from oracle import install_stubs
    return install_stubs.reference_available()


@pytest.mark.skipif(not _reference_available(), reason="needs the reference tree")
def test_reference_create_new_model_builds_this_package_model_for_ship_tensorf():
    """compat.install_model_classes(): the reference's create_new_model with configs/nerf/ship.tensorf.py's fine_model_and_render
    values (at a reduced num_voxels) constructs this package's DirectVoxGO instead of raising"""
    import types
    from oracle import install_stubs
    from unboundednerfpytorch_amd import compat, grid, voxgo_model
    import sys
    install_stubs.install()
    if 'tkinter' not in sys.modules:             # (the reference's load_waymo.py imports a name from it by accident; never used)
        tk, tix = types.ModuleType('tkinter'), types.ModuleType('tkinter.tix')
        tk.image_names, tk.tix, tk.__path__, tix.HList = None, tix, [], None
        sys.modules['tkinter'], sys.modules['tkinter.tix'] = tk, tix
    ted = sys.modules.get('torch_efficient_distloss')
    if ted is not None and not hasattr(ted, 'flatten_eff_distloss'):          # (a placeholder of install_stubs: run_train.py imports the name)
        from unboundednerfpytorch_amd.ops import flatten_eff_distloss
        ted.flatten_eff_distloss = flatten_eff_distloss
    orig = compat.install_model_classes()
    try:
        rt = install_stubs.import_reference("run_train")
        cfg_model = dict(num_voxels_density=24 ** 3, num_voxels_rgb=24 ** 3, num_voxels_base_rgb=24 ** 3, alpha_init=1e-2,
                         fast_color_thres=1e-4, rgbnet_dim=12, rgbnet_direct=True, **TENSORF_KW)
        cfg_train = types.SimpleNamespace(pg_scale=[1000], lrate_density=0.02, lrate_k0=0.02, lrate_rgbnet=1e-3, lrate_decay=20,
                                          skip_zero_grad_fields=['density', 'k0'])
        cfg_train.keys = lambda: [k for k in vars(cfg_train) if k != 'keys']
        cfg = types.SimpleNamespace(data=types.SimpleNamespace(dataset_type='blender', ndc=False, unbounded_inward=False), model='DVGO')
        args = types.SimpleNamespace(sample_num=-1, block_num=1)
        model, opt = rt.create_new_model(args, cfg, cfg_model, cfg_train, torch.tensor([-1., -1, -1]), torch.tensor([1., 1, 1]), 'fine', None, 'cpu')
        assert type(model) is voxgo_model.DirectVoxGO and isinstance(model.k0, grid.TensoRFGrid)
        assert model.k0.f_vec.shape == (72, 12) and model.density.xy_plane.shape[1] == 8
    finally:
        import importlib
        importlib.import_module("FourierGrid.dvgo").DirectVoxGO, importlib.import_module("FourierGrid.dcvgo").DirectContractedVoxGO, \
            importlib.import_module("FourierGrid.FourierGrid_model").FourierGridModel = orig


def test_tensorf_kernels_keep_everything_in_registers():
    """Build quality (no GPU needed, reads the built library): the four new kernels have no VGPR or SGPR spills and no scratch, and
    stay inside the occupancy DESIGN.md 4.6 states -- query <= 80 VGPR (6 waves per SIMD), backward <= 98 (5), bake and TV <= 64 (8)"""
    import test_capi
    from unboundednerfpytorch_amd import _lib
    meta = test_capi._kernel_metadata(_lib.LIB_PATH)
    budget = {"_Z15k_tensorf_queryILb": 80, "_Z24k_tensorf_query_backwardILb": 98, "_Z14k_tensorf_bakeILb": 64, "_Z12k_tensorf_tvILb": 64}
    for prefix, limit in budget.items():
        ks = [k for k in meta if k.startswith(prefix)]
        assert ks, prefix
        for k in ks:
            m = meta[k]
            assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0 and m.get("private_segment_fixed_size", 0) == 0, (k, m)
            assert m["vgpr_count"] <= limit, (k, m)
