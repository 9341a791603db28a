"""The native training step of the forward-facing model (native_step.VoxGOStep mode 'mpi', ugrid_voxgo_step mode 3) -- HOST side, on
the CPU: the struct fill over a stand-in library, both backward routes, which DirectMPIGO configurations select the native step,
where the new struct fields lie, and the identity that lets the compaction's table lookup stand for the reference's
s = (step_id + 0.5) / N_samples.  The kernels' results are tests/test_gpu_mpi_native.py's business."""
import ctypes

import pytest
import torch

import mpi_cases


def model(**kw):
    from unboundednerfpytorch_amd.mpi_model import DirectMPIGO
    args = dict(xyz_min=mpi_cases.XYZ_MIN, xyz_max=mpi_cases.XYZ_MAX, num_voxels=9600, mpi_depth=24,
                fast_color_thres=mpi_cases.fast_color_thres(0.5, 24), rgbnet_dim=9, rgbnet_depth=3, rgbnet_width=64, viewbase_pe=0)
    args.update(kw)
    return DirectMPIGO(**args)


def test_native_step_host_side_runs_over_a_stand_in_library_for_mpi(monkeypatch):
    """tests/test_host_logic.py::test_native_step_host_side_runs_over_a_stand_in_library for 'mpi': the C entry points replaced by a
    stand-in that only fills M1 / M2, CPU tensors, strided views as ray inputs -- what the struct carries (mode 3, slots = n_steps, the
    shift table's own address, the s table, the mask, scalar shift 0), the outputs' shapes, both backward routes, a bad target"""
    from unboundednerfpytorch_amd import _lib, native_step
    calls = []
    m = model()
    R, n_steps = 8, m.n_samples(0.5)
    assert n_steps == 47

    class StandIn:
        def ugrid_voxgo_step_sample(self, ps, st):
            s = ctypes.cast(ps, ctypes.POINTER(_lib.VoxgoStep)).contents
            assert s.mode == 3 and s.n_rays == R and s.slots == n_steps and s.mpi_depth == 24
            assert s.plane_shift == m.act_shift.grid.data_ptr()
            assert s.t_table and s.mask and list(s.mask_dims) == list(m.mask_cache.mask.shape)
            assert (s.C, s.pe, s.width) == (9, 0, 64) and s.act_shift == 0.0
            assert (s.P, s.kP, s.freq_num, s.k0_freq_num, s.k0_channels_last) == (1, 1, 0, 0, 0)
            assert (s.X, s.Y, s.Z) == tuple(m.world_size.tolist()) == (s.kX, s.kY, s.kZ)
            assert s.sync_free == 0 and s.coef9[4] == 0.0 and s.coef9[2] == pytest.approx(0.01)
            s.M1, s.M2 = 40, 17
            calls.append("sample")
            return 0

        def ugrid_voxgo_step_ws_floats(self, ps):
            return 1000

        def ugrid_voxgo_step_bwd_ws_floats(self, ps):
            return 1000

        def __getattr__(self, name):
            if name.startswith("ugrid_voxgo_step_"):
                def f(ps, st, _n=name[len("ugrid_voxgo_step_"):]):
                    s = ctypes.cast(ps, ctypes.POINTER(_lib.VoxgoStep)).contents
                    assert s.ws and s.logits and s.weights2 and s.t2 and not s.inner2
                    assert _n == "forward" or (s.grad_loss and s.ws_bwd and s.grad_k0_grid and s.g_w2 and not s.touch)
                    calls.append(_n)
                    return 0
                return f
            raise AttributeError(name)

    monkeypatch.setattr(native_step, "_L", StandIn())
    monkeypatch.setattr(_lib, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_lib, "require_cuda_grid", lambda *a: _lib.is_channels_last(a[0][1]))
    monkeypatch.setattr(_lib, "stream_of", lambda t: None)
    monkeypatch.setattr(_lib, "guard", lambda d: _lib._NO_GUARD)
    monkeypatch.setattr(_lib, "empty_like_grid", lambda shape, cl, dev, zero=False: torch.zeros(shape).contiguous(
        memory_format=torch.channels_last_3d if cl else torch.contiguous_format))
    cfg = {"mode": "mpi", "interval": 0.5 * m.voxel_size_ratio, "thres": m.fast_color_thres, "mask_scale": [1., 1., 1.],
           "mask_shift": [0., 0., 0.], "n_steps": n_steps, "mpi_depth": 24, "act_shift": m.act_shift.get_dense_grid().detach().reshape(-1)}
    params = m._native_params()

    def pack(**over):
        p = {"mode": "mpi", "cfg": cfg, "t": m.sample_table(0.5, "cpu"), "rays_o": torch.zeros(R, 3), "rays_d": torch.ones(R, 6)[:, ::2],
             "viewdirs": torch.ones(3, R).t(), "viewfreq": m.viewfreq, "xyz_min": m.xyz_min, "xyz_max": m.xyz_max, "k0_xyz_min": m.k0.xyz_min,
             "k0_xyz_max": m.k0.xyz_max, "mask": m.mask_cache.mask, "target": torch.zeros(R, 3), "bg": torch.rand(R, 3),
             "coef": (1, 0.001, 0.01, 0.01, 0, 0, 1 / n_steps, R, 0)}
        p.update(over)
        return p
    pk = pack()
    loss, mse = native_step.VoxGOStep.apply(*params, pk)
    assert loss.requires_grad and not mse.requires_grad and loss.shape == mse.shape == ()
    out = pk["out"]
    assert out["weights"].shape == out["ray_id"].shape == out["t"].shape == (17,) and out["raw_logits"].shape == (17, 3)
    assert out["loss_mse"].shape == (2,) and out["alphainv_last"].shape == (R,) and out["rgb_marched"].shape == (R, 3) and out["inner"] is None
    loss.backward()
    assert all(p.grad is not None and p.grad.shape == p.shape for p in params) and m.act_shift.grid.grad is None
    assert calls == ["sample", "forward", "backward"]
    # the mid-backward route: the callback sees the k0 gradient assigned, the node returns none for k0
    del calls[:]
    for p in params:
        p.grad = None
    pk = pack()
    seen = []
    pk["k0_grad_ready"] = lambda prm: seen.append((prm is m.k0.grid, prm.grad is not None))
    native_step.VoxGOStep.apply(*params, pk)[0].backward()
    assert seen == [(True, True)] and calls == ["sample", "forward", "backward_k0", "backward_density"]
    assert m.k0.grid.grad is not None and m.density.grid.grad is not None
    # ... and not over a gradient that is already accumulated
    del calls[:], seen[:]
    pk = pack()
    pk["k0_grad_ready"] = lambda prm: seen.append(1)
    native_step.VoxGOStep.apply(*params, pk)[0].backward()
    assert seen == [] and calls[-1] == "backward"
    with pytest.raises(RuntimeError, match=r"\[R,3\]"):
        native_step.VoxGOStep.apply(*params, pack(target=torch.zeros(R + 1, 3)))
    # grid.TrainSampleVox's limits for 'mpi', and the s table has to have n_steps entries
    for bad_cfg in (dict(cfg, n_steps=1), dict(cfg, mpi_depth=257), dict(cfg, act_shift=torch.zeros(23))):
        with pytest.raises(RuntimeError, match="mpi"):
            native_step.VoxGOStep.apply(*params, pack(cfg=bad_cfg))
    with pytest.raises(RuntimeError, match="s table"):
        native_step.VoxGOStep.apply(*params, pack(t=m.sample_table(0.5, "cpu")[:-1]))


def test_native_step_selection_for_mpi_is_host_logic():
    """the fine stage with the default rgbnet selects the native step (TrainModel._native_params), its eight parameters are the two
    grids and the rgbnet's -- never the per-plane shift --; the coarse stage, another rgbnet depth, no_grad, a frozen grid and
    native_step = False select the op-by-op ops"""
    m = model()
    assert m.native_step is True
    p = m._native_params()
    assert p is not None and len(p) == 8 and p[0] is m.density.grid and p[1] is m.k0.grid
    assert all(q is not m.act_shift.grid for q in p) and not m.act_shift.grid.requires_grad
    assert [tuple(q.shape) for q in p[2:]] == [(64, 12), (64,), (64, 64), (64,), (3, 64), (3,)]
    assert model(rgbnet_dim=0)._native_params() is None             # coarse stage: no rgbnet
    assert model(rgbnet_depth=4)._native_params() is None           # not the default network
    with torch.no_grad():
        assert m._native_params() is None
    m.density.grid.requires_grad_(False)
    assert m._native_params() is None
    m.density.grid.requires_grad_(True)
    assert m._native_params() is not None
    m.native_step = False
    assert m._native_params() is None


def test_new_struct_fields_lie_after_the_old_ones():
    """mode 3's fields are appended: no field of the modes 0-2 moved"""
    from unboundednerfpytorch_amd import _lib
    S = _lib.VoxgoStep
    assert S.plane_shift.offset > S.touch.offset and S.mpi_depth.offset > S.plane_shift.offset
    assert [n for n, _ in S._fields_][-3:] == ["touch", "plane_shift", "mpi_depth"]
    assert S.touch.offset + ctypes.sizeof(ctypes.c_void_p) == S.plane_shift.offset


def test_s_table_equals_the_references_expression():
    """the native step's t2 = table[step] with table = (arange(n, float32) + 0.5) / n (DirectMPIGO.sample_table) against the
    reference's s = (step_id + 0.5) / N_samples with an int64 step_id (dmpigo.py:319): the same float32 for every step of every
    n_steps the step accepts up to 512 (mpi_depth 256 at stepsize 0.5 gives 511)"""
    for n in range(2, 513):
        table = (torch.arange(n, dtype=torch.float32) + 0.5) / n
        ref = (torch.arange(n, dtype=torch.int64) + 0.5) / n
        assert ref.dtype == torch.float32 and torch.equal(table, ref), n
    m = model()
    assert torch.equal(m.sample_table(0.5, "cpu"), (torch.arange(47, dtype=torch.int64) + 0.5) / 47)
