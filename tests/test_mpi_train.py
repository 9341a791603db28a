"""mpi_model.DirectMPIGO -- the TRAINING counterpart of the reference's forward-facing model (dmpigo.py:18-340) -- host side, on
the CPU, against the fixtures the reference's own classes wrote (tests/golden/gen_mpi_train_golden.py): parameter / buffer names
and shapes, get_kwargs keys, the initial per-plane shift, the derived sizes, the NDC ray tables, checkpoints both ways, the class
rebinding for the reference's training program, and the per-axis total-variation weights through train_iteration's tv_terms.
The model has no CPU forward; tests/test_gpu_mpi_train.py covers the kernels."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import mpi_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
GOLD = os.path.join(ROOT, "tests", "golden")
IDS = [c[0] for c in mpi_cases.MPI_CASES]


def build(case, device="cpu"):
    """the model of an MPI_CASES row holding the row's synthetic parameters, its rays and render kwargs"""
    from unboundednerfpytorch_amd.mpi_model import DirectMPIGO
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    m = DirectMPIGO(xyz_min=mpi_cases.XYZ_MIN, xyz_max=mpi_cases.XYZ_MAX, num_voxels=nvox, mpi_depth=D,
                    fast_color_thres=mpi_cases.fast_color_thres(stepsize, D), rgbnet_dim=C, rgbnet_depth=3,
                    rgbnet_width=mpi_cases.RGBNET_WIDTH, viewbase_pe=0)
    ws = [int(x) for x in m.world_size]
    sd = m.state_dict()
    with torch.no_grad():
        for k, val in mpi_cases.mpi_params(seed, ws, C, dm, ds).items():
            assert tuple(sd[k].shape) == tuple(val.shape), (k, sd[k].shape, val.shape)
            sd[k].copy_(torch.from_numpy(val))
    m = m.to(device)
    o, d, v = [torch.from_numpy(a).to(device) for a in mpi_cases.ndc_rays(seed, R)]
    return m, (o, d, v), dict(near=0, far=1, stepsize=stepsize, bg=1, render_depth=True)


def fresh(case):
    from unboundednerfpytorch_amd.mpi_model import DirectMPIGO
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    return DirectMPIGO(xyz_min=mpi_cases.XYZ_MIN, xyz_max=mpi_cases.XYZ_MAX, num_voxels=nvox, mpi_depth=D,
                       fast_color_thres=mpi_cases.fast_color_thres(stepsize, D), rgbnet_dim=C, rgbnet_depth=3,
                       rgbnet_width=mpi_cases.RGBNET_WIDTH, viewbase_pe=0)


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=IDS)
def test_names_shapes_kwargs_and_initial_shift_are_the_references(case):
    m = fresh(case)
    gold = np.load(os.path.join(GOLD, "mpi_train_" + case[0] + ".npz"))
    sd = m.state_dict()
    assert sorted(sd.keys()) == gold["sd_keys"].tolist()
    assert [str(tuple(sd[k].shape)) for k in sorted(sd.keys())] == gold["sd_shapes"].tolist()
    assert sorted(m.get_kwargs().keys()) == gold["kwargs_keys"].tolist()
    assert np.array_equal(sd["act_shift.grid"].numpy(), gold["fresh_act_shift"])        # the float64 recipe, one rounding
    assert not m.act_shift.grid.requires_grad and m.density.grid.requires_grad and m.k0.grid.requires_grad
    assert [n for n, p in m.named_parameters() if p.requires_grad and n.startswith("act_shift")] == []
    if case[4] > 0:
        assert m.viewfreq.numel() == 0 and m.rgbnet[0].in_features == case[4] + 3
        assert m.k0.grid.is_contiguous()             # C = 9: canonical layout


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=IDS)
def test_derived_sizes_and_no_cpu_forward(case):
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    m, (o, d, v), kw = build(case)
    gold = np.load(os.path.join(GOLD, "mpi_train_" + name + ".npz"))
    assert m.world_size.tolist() == gold["world_size"].tolist() == mpi_cases.world_size(nvox, D)
    assert m.world_size_density is m.world_size and m.world_size_rgb is m.world_size
    assert m.voxel_size_ratio == 256. / D and np.float32(m.voxel_size_ratio) == gold["ratio"] and m.mpi_depth == D      # (stored as fp32)
    assert m.n_samples(stepsize) == int(gold["n_max"]) == int((D - 1) / stepsize) + 1
    t = m.sample_table(stepsize, "cpu")
    assert t.numel() == int(gold["n_max"]) and t.dtype == torch.float32
    k = m.get_kwargs()
    assert k["num_voxels"] == nvox and k["mpi_depth"] == D and k["mask_cache_world_size"] == list(m.mask_cache.mask.shape)
    with pytest.raises(RuntimeError):                # no CPU path: the ops need the HIP library and device tensors
        m(o[:4], d[:4], v[:4], **kw)
    m.act_shift -= 0.25                              # run_train.py:200 (`model.act_shift -= decay_after_scale`)
    want = mpi_cases.mpi_params(seed, m.world_size.tolist(), C, dm, ds)["act_shift.grid"] - np.float32(0.25)
    assert np.array_equal(m.act_shift.grid.numpy(), want) and isinstance(m.act_shift, torch.nn.Module)


def test_ndc_ray_tables_equal_the_reference_functions_on_cpu():
    import gen_mpi_train_golden as gen
    from unboundednerfpytorch_amd import train_rays as tr
    g = np.load(os.path.join(GOLD, "mpi_train_rays.npz"))
    imgs, poses, HW, Ks = gen.ray_scene()
    flags = dict(inverse_y=False, flip_x=False, flip_y=True)
    r = tr.get_training_rays_ndc(rgb_tr=imgs, train_poses=poses, HW=HW, Ks=Ks, **flags)
    for k, t in zip(("rgb", "o", "d", "v"), r[:4]):
        assert np.array_equal(t.numpy(), g["img_" + k]), k
    assert list(r[4]) == g["img_imsz"].tolist()
    r = tr.get_training_rays_flatten_ndc(rgb_tr_ori=list(imgs), train_poses=poses, HW=HW, Ks=Ks, **flags)
    for k, t in zip(("rgb", "o", "d", "v"), r[:4]):
        assert np.array_equal(t.numpy(), g["flat_" + k]), k
    assert list(r[4]) == g["flat_imsz"].tolist()
    # NDC origins lie on the near plane z = -1 and move with the pixel: not the rays of ndc=False
    assert np.allclose(g["flat_o"][:, 2], -1.0, atol=1e-6)
    r0 = tr.get_training_rays_flatten(rgb_tr_ori=list(imgs), train_poses=poses, HW=HW, Ks=Ks, ndc=False, **flags)
    assert not np.allclose(r0[1].numpy(), g["flat_o"])
    for fn, kw in ((tr.get_training_rays, dict(rgb_tr=imgs)), (tr.get_training_rays_flatten, dict(rgb_tr_ori=list(imgs))),
                   (tr.FourierGrid_get_training_rays, dict(rgb_tr_ori=list(imgs)))):
        with pytest.raises(NotImplementedError):     # the general functions keep refusing ndc=True
            fn(train_poses=poses.clone(), HW=HW, Ks=Ks, ndc=True, **flags, **kw)


def test_checkpoints_interchange_with_the_renderer_and_the_reference():
    from unboundednerfpytorch_amd import mpi_render
    from unboundednerfpytorch_amd.mpi_model import DirectMPIGO
    case = mpi_cases.MPI_CASES[0]
    m, _, _ = build(case)
    ckpt = {"model_kwargs": m.get_kwargs(), "model_state_dict": m.state_dict()}
    st = mpi_render.mpi_state_from_reference_checkpoint(ckpt)          # this model's checkpoint -> the renderer's state
    want = mpi_cases.state(case)
    for k in ("density_grid", "act_shift", "k0_grid", "mask", "xyz2ijk_scale", "xyz2ijk_shift", "xyz_min", "xyz_max", "world_size"):
        assert torch.equal(torch.as_tensor(st[k]), torch.as_tensor(want[k])), k
    for a, b in zip(st["rgbnet_weights"] + st["rgbnet_biases"], want["rgbnet_weights"] + want["rgbnet_biases"]):
        assert torch.equal(a, b)
    assert st["mpi_depth"] == want["mpi_depth"] and st["voxel_size_ratio"] == want["voxel_size_ratio"]
    assert st["fast_color_thres"] == want["fast_color_thres"] and st["viewbase_pe"] == 0
    # the reference's own checkpoint (tests/golden/mpi_ckpt_small.tar, written by dmpigo.DirectMPIGO) -> this model, strictly
    ref = torch.load(os.path.join(GOLD, "mpi_ckpt_small.tar"), map_location="cpu", weights_only=False)
    m2 = DirectMPIGO(**ref["model_kwargs"])
    m2.load_state_dict(ref["model_state_dict"], strict=True)
    sd = m2.state_dict()
    assert sorted(sd.keys()) == sorted(ref["model_state_dict"].keys())
    for k, t in ref["model_state_dict"].items():
        assert torch.equal(sd[k], t), k
    kw2 = m2.get_kwargs()
    assert sorted(kw2.keys()) == sorted(ref["model_kwargs"].keys())
    for k, val in ref["model_kwargs"].items():
        assert np.array_equal(np.asarray(kw2[k]), np.asarray(val)), k


def test_install_mpi_model_class_rebinds_the_reference_class(monkeypatch):
    """compat.install_mpi_model_class on stand-in modules registered under the reference's names (nothing outside the repository):
    `FourierGrid.dmpigo.DirectMPIGO` then is this package's model, built with create_new_model's call shape (run_train.py:37-41)"""
    from unboundednerfpytorch_amd import compat, mpi_model
    pkg = types.ModuleType("FourierGrid")
    pkg.__path__ = []
    monkeypatch.setitem(sys.modules, "FourierGrid", pkg)
    dm = types.ModuleType("FourierGrid.dmpigo")
    dm.DirectMPIGO = type("DirectMPIGO", (torch.nn.Module,), {})
    pkg.dmpigo = dm
    monkeypatch.setitem(sys.modules, dm.__name__, dm)
    run_train = types.ModuleType("FourierGrid.run_train")
    run_train.dmpigo = dm                                  # run_train.py:9 imports the module, not the class
    stand_in = dm.DirectMPIGO
    orig = compat.install_mpi_model_class()
    assert orig is stand_in and dm.DirectMPIGO is mpi_model.DirectMPIGO and run_train.dmpigo.DirectMPIGO is mpi_model.DirectMPIGO
    extra = dict(num_voxels_base=8 ** 3, density_type='DenseGrid', k0_type='DenseGrid', density_config={}, k0_config={}, mpi_depth=16,
                 nearest=False, pre_act_density=False, in_act_density=False, bbox_thres=1e-3, mask_cache_thres=1e-3, rgbnet_dim=9,
                 rgbnet_full_implicit=False, rgbnet_direct=True, rgbnet_depth=3, rgbnet_width=64, alpha_init=1e-2,
                 fast_color_thres=1e-3, maskout_near_cam_vox=False, world_bound_scale=1.0, stepsize=0.5)
    m = run_train.dmpigo.DirectMPIGO(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=16 * 10 * 10, **extra)
    assert isinstance(m, mpi_model.DirectMPIGO) and m.world_size.tolist() == [10, 10, 16]
    dm.DirectMPIGO = orig
    assert dm.DirectMPIGO is stand_in


def test_tv_hook_is_uniform_for_the_old_models_and_per_axis_for_mpi():
    from unboundednerfpytorch_amd import fourier_model, voxgo_model
    w = 1e-5 / 4096
    dv = voxgo_model.DirectVoxGO(xyz_min=[-1, -0.8, -1.1], xyz_max=[1, 0.9, 1], num_voxels=10 ** 3, num_voxels_base=10 ** 3,
                                 alpha_init=1e-2, fast_color_thres=1e-4)
    dc = voxgo_model.DirectContractedVoxGO(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=9 ** 3, num_voxels_base=9 ** 3,
                                           alpha_init=1e-2, fast_color_thres=1e-4)
    fg = fourier_model.FourierGridModel(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels_density=8 ** 3, num_voxels_base_density=8 ** 3,
                                        num_voxels_rgb=6 ** 3, num_voxels_base_rgb=6 ** 3, num_voxels_viewdir=-1, alpha_init=1e-3,
                                        fast_color_thres=1e-4, fourier_freq_num=1, rgbnet_dim=12)
    for m in (dv, dc, fg):
        for which, ws in (("density", m.world_size_density), ("k0", m.world_size_rgb)):
            was = float(w * ws.max() / 128)          # what train_iteration put into tv_terms before the hook existed
            assert m.tv_axis_weights(w, which) == (was, was, was)
    assert fg.tv_axis_weights(w, "density") != fg.tv_axis_weights(w, "k0")
    m = fresh(mpi_cases.MPI_CASES[0])                # world [20, 19, 24]
    wxy, wz = float(w * m.world_size[:2].max() / 128), float(w * m.mpi_depth / 128)
    assert m.tv_axis_weights(w, "density") == m.tv_axis_weights(w, "k0") == (wxy, wxy, wz) and wxy != wz
    # the model's own TV methods (dmpigo.py:209-217) hand the same triple to the grid
    calls = []
    m.density.grad = None
    m.density.tv_module = types.SimpleNamespace(total_variation_add_grad=lambda p, g, wx, wy, wz_, dense: calls.append((wx, wy, wz_, dense)))
    m.density_total_variation_add_grad(w, True)
    assert calls == [(wxy, wxy, wz, True)]


def test_scalar_and_triple_tv_terms_give_identical_updates_and_axes_are_distinguished():
    """ShardedMaskedAdam.step(tv_terms=...) over the oracle back-end: (w, dense, tv) and ((w, w, w), dense, tv) update bit for bit
    alike in the dense and in the masked TV mode; a per-axis triple equals the plain `TV with (wx, wy, wz), then Adam` sequence"""
    from oracle import ref_ops
    from unboundednerfpytorch_amd.sharded_adam import ShardedMaskedAdam
    tv = types.SimpleNamespace(total_variation_add_grad=ref_ops.total_variation_add_grad)
    g0 = torch.Generator().manual_seed(3)
    p0 = torch.randn(1, 3, 5, 4, 6, generator=g0)
    grads = [torch.randn(p0.shape, generator=g0) * (torch.rand(p0.shape, generator=g0) > 0.5) for _ in range(2)]

    def run(weight):
        p = torch.nn.Parameter(p0.clone())
        opt = ShardedMaskedAdam([{'params': [p], 'lr': 0.1, 'skip_zero_grad': True}], ops=ref_ops)
        for step in range(2):
            p.grad = grads[step].clone()
            opt.step(tv_terms={p: (weight, step == 0, tv)})
        return p.detach().clone()
    assert torch.equal(run(1e-2), run((1e-2, 1e-2, 1e-2)))
    assert torch.equal(run(1e-2), run([1e-2, 1e-2, 1e-2]))
    got = run((1e-2, 1e-2, 3e-2))
    assert not torch.equal(got, run(1e-2))
    r, m_, v_ = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(2):
        g = grads[step].clone()
        ref_ops.total_variation_add_grad(r, g, 1e-2, 1e-2, 3e-2, step == 0)
        ref_ops.masked_adam_upd(r, g, m_, v_, step + 1, 0.9, 0.99, 0.1, 1e-8)
    assert torch.equal(got, r)


def test_train_iteration_hands_the_models_triple_to_the_optimizer():
    """train_step.train_iteration builds tv_terms from the model's hook: a stand-in model and optimizer record what arrives"""
    from unboundednerfpytorch_amd import train_step as ts

    class Grid(torch.nn.Module):
        tv_module = None

        def __init__(self):
            super().__init__()
            self.grid = torch.nn.Parameter(torch.zeros(1, 1, 2, 2, 2))

    class Model(torch.nn.Module):
        def __init__(self, hook):
            super().__init__()
            self.density, self.k0 = Grid(), Grid()
            self.world_size_density = self.world_size_rgb = torch.tensor([20, 19, 24])
            if hook:
                self.tv_axis_weights = lambda w, which: (w * 2, w * 2, w * 3) if which == 'density' else (w, w, w * 5)

        def forward(self, o, d, v, **kw):
            rgb = (self.density.grid.sum() + self.k0.grid.sum()) * torch.ones(o.shape[0], 3)
            return {'rgb_marched': rgb, 'alphainv_last': torch.full((o.shape[0],), 0.5)}

    class Opt:
        param_groups = []

        def zero_grad(self, set_to_none=True):
            pass

        def step(self, tv_terms=None):
            self.seen = tv_terms
    cfg = dict(weight_main=1.0, tv_every=1, tv_after=0, tv_before=10, tv_dense_before=10, weight_tv_density=1e-3, weight_tv_k0=1e-4,
               lrate_decay=20)
    o = torch.zeros(8, 3)
    for hook in (True, False):
        m, opt = Model(hook), Opt()
        ts.train_iteration(m, opt, o, o, o, torch.zeros(8, 3), cfg, 1, {})
        wd, wk = opt.seen[m.density.grid][0], opt.seen[m.k0.grid][0]
        if hook:
            assert wd == (1e-3 / 8 * 2, 1e-3 / 8 * 2, 1e-3 / 8 * 3) and wk == (1e-4 / 8, 1e-4 / 8, 1e-4 / 8 * 5)
        else:                                        # a model without the hook: the single weight, as before
            assert wd == float(1e-3 / 8 * torch.tensor(24) / 128) and wk == float(1e-4 / 8 * torch.tensor(24) / 128)
        assert opt.seen[m.density.grid][1] is True


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=IDS)
def test_op_by_op_chain_over_the_oracle_backend_reproduces_the_reference(case):
    """the model's host logic on the CPU: with the C oracle injected for the extension modules (backend=, the hook FourierGridModel
    has), the op-by-op forward + backward, update_occupancy_cache and scale_volume_grid give the reference's results BIT FOR BIT --
    the same torch ops on the same inputs in the same order (one thread, like the generator)"""
    from test_fourier_model import oracle_backend
    from unboundednerfpytorch_amd.mpi_model import DirectMPIGO
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        m = DirectMPIGO(xyz_min=mpi_cases.XYZ_MIN, xyz_max=mpi_cases.XYZ_MAX, num_voxels=nvox, mpi_depth=D,
                        fast_color_thres=mpi_cases.fast_color_thres(stepsize, D), rgbnet_dim=C, rgbnet_depth=3,
                        rgbnet_width=mpi_cases.RGBNET_WIDTH, viewbase_pe=0, backend=oracle_backend())
        assert not m.fused_forward and not m.fused_loss
        sd = m.state_dict()
        with torch.no_grad():
            for k, val in mpi_cases.mpi_params(seed, m.world_size.tolist(), C, dm, ds).items():
                sd[k].copy_(torch.from_numpy(val))
        o, d, v = [torch.from_numpy(a) for a in mpi_cases.ndc_rays(seed, R)]
        kw = dict(near=0, far=1, stepsize=stepsize, bg=1, render_depth=True)
        gold = np.load(os.path.join(GOLD, "mpi_train_" + name + ".npz"))
        out = m(o, d, v, global_step=1, **kw)
        target = torch.from_numpy(gold["target"])
        loss = torch.nn.functional.mse_loss(out["rgb_marched"], target)
        p = out["alphainv_last"].clamp(1e-6, 1 - 1e-6)
        loss = loss + 0.01 * (-(p * torch.log(p) + (1 - p) * torch.log(1 - p))).mean()
        loss = loss + 0.05 * (out["weights"] * out["weights"]).sum() / R
        loss.backward()
        assert out["n_max"] == int(gold["n_max"]) and int(gold["n_kept"]) >= 500
        for k in ("weights", "raw_alpha", "raw_rgb", "ray_id", "s", "rgb_marched", "alphainv_last", "depth"):
            assert np.array_equal(out[k].detach().numpy(), gold[k]), k
        assert float(loss.detach()) == float(gold["loss"])
        for k, q in m.named_parameters():
            if ("grad." + k) in gold.files:
                assert np.array_equal(q.grad.numpy(), gold["grad." + k]), k
            else:
                assert q.grad is None and k == "act_shift.grid"
        m.zero_grad()
        m.update_occupancy_cache()
        assert np.array_equal(m.mask_cache.mask.numpy(), gold["occ_mask"])
        m.scale_volume_grid(2 * nvox, D)
        assert m.world_size.tolist() == gold["scaled_world_size"].tolist()
        assert np.array_equal(m.density.grid.detach().numpy(), gold["scaled_density"])
        assert np.array_equal(m.k0.grid.detach().numpy()[:, gold["scaled_k0_channels"].tolist()], gold["scaled_k0"])
        assert np.array_equal(m.k0.grid.detach().numpy()[:, gold["scaled_k0_rest_channels"].tolist()].astype(np.float16),
                              gold["scaled_k0_rest_f16"])
        assert np.array_equal(m.mask_cache.mask.numpy(), gold["scaled_mask"])
        with torch.no_grad():
            out2 = m(o, d, v, global_step=2, **kw)
        assert out2["weights"].numel() == int(gold["scaled_n_kept"])
        assert np.array_equal(out2["rgb_marched"].numpy(), gold["scaled_rgb_marched"])
    finally:
        torch.set_num_threads(threads)
