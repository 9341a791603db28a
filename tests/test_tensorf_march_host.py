"""Host side of the fused sampling march over a TensoRF density (no GPU needed): the two C entry points are declared, exported and
bound; every k_train_march_tensorf instantiation keeps its state in registers within the occupancy DESIGN.md 4.6 states; the autograd
op refuses host tensors and mixed factor layouts before any library call; the model switch exists and is off."""
import ctypes
import re

import pytest
import torch

import tensorf_cases as tc

NEW_SYMBOLS = ("ugrid_train_sample_dvgo_tensorf", "ugrid_train_sample_dcvgo_tensorf")
MARCH_VGPR_BUDGET = 80          # <= 80 VGPR, 6 waves per SIMD


def test_the_two_entry_points_are_declared_exported_and_bound():
    import test_capi
    from unboundednerfpytorch_amd import _lib
    declared = test_capi.declared_functions()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    # the dense twins' argument lists with `density_grid` replaced by six factor pointers and R, Rxy, comp_last added to X, Y, Z
    for name in NEW_SYMBOLS:
        dense, tf = _lib._SIGNATURES[name[:-len("_tensorf")]], _lib._SIGNATURES[name]
        assert tf[0] is dense[0] and len(tf[1]) == len(dense[1]) + 8
        assert tf[1][:12] == [ctypes.c_void_p] * 6 + [ctypes.c_int] * 6 and tf[1][12:] == dense[1][4:]


def test_entry_points_refuse_bad_factors_before_any_launch():
    """hipErrorInvalidValue (1) for a null factor, R < 1, Rxy < 1 or a dimension < 1 -- host checks, made before the ray count is looked
    at and before anything touches a device"""
    from unboundednerfpytorch_amd import _lib
    L = _lib.load()
    P = 4096                        # a non-null value: never dereferenced, the checks come first
    tail_dvgo = [None, None, 0, 8, None, None, 0.2, 1e9, 0.1, None, None, None, None, 0.0, 0.5, 1e-4] + [None] * 9
    tail_dcvgo = [None, None, 0, None, 8, None, None, None, None, 0.2, 0, 0.1, None, None, None, None, 0.0, 0.5, 1e-4] + [None] * 9
    for fn, tail in ((L.ugrid_train_sample_dvgo_tensorf, tail_dvgo), (L.ugrid_train_sample_dcvgo_tensorf, tail_dcvgo)):
        assert fn(*[P] * 6, 5, 7, 9, 3, 2, 0, *tail) == 0                       # well-formed, no rays: nothing to do
        for k in range(6):
            ptrs = [P] * 6
            ptrs[k] = None
            assert fn(*ptrs, 5, 7, 9, 3, 2, 0, *tail) == 1, k
        for dims in ((0, 7, 9, 3, 2), (5, 0, 9, 3, 2), (5, 7, 0, 3, 2), (5, 7, 9, 0, 2), (5, 7, 9, 3, 0), (5, 7, 9, -1, 2)):
            assert fn(*[P] * 6, *dims, 0, *tail) == 1, dims


def test_march_kernels_keep_everything_in_registers():
    """the four instantiations (DirectContractedVoxGO / DirectVoxGO x canonical / component-last): no VGPR or SGPR spill, no private
    segment, and at most the VGPR count DESIGN.md 4.6 states"""
    import test_capi
    from unboundednerfpytorch_amd import _lib
    meta = test_capi._kernel_metadata(_lib.LIB_PATH)
    ks = sorted(k for k in meta if k.startswith("_Z21k_train_march_tensorfILi"))
    assert [re.match(r"_Z21k_train_march_tensorfILi(\d)ELb([01])E", k).groups() for k in ks] == [("1", "0"), ("1", "1"), ("2", "0"), ("2", "1")], ks
    for k in ks:
        m = meta[k]
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0 and m.get("private_segment_fixed_size", 0) == 0, (k, m)
        assert m["vgpr_count"] <= MARCH_VGPR_BUDGET, (k, m)
    design = open(test_capi.ROOT + "/DESIGN.md").read()
    assert re.search(r"k_train_march_tensorf[^\n]*<= %d VGPR" % MARCH_VGPR_BUDGET, design)          # the figure the document states


def _cpu_factors(comp_last=()):
    g = torch.Generator().manual_seed(1)
    out = []
    for name, shp in tc.shapes((5, 7, 9), 3, 2, 1).items():
        t = torch.randn(shp, generator=g)
        out.append(t.contiguous(memory_format=torch.channels_last) if name in comp_last else t)
    return out


def _op_args():
    o = torch.zeros(4, 3)
    cfg = {'mode': 'dvgo', 'act_shift': 0.0, 'interval': 0.5, 'thres': 1e-4, 'mask_scale': [1, 1, 1], 'mask_shift': [0, 0, 0], 'near': 0.2,
           'far': 1e9, 'stepdist': 0.1, 'slots': 8}
    return o, o.clone(), None, torch.tensor(tc.XYZ_MIN), torch.tensor(tc.XYZ_MAX), torch.ones(2, 2, 2, dtype=torch.bool), cfg


def test_op_refuses_host_tensors_and_mixed_layouts_before_any_library_call(monkeypatch):
    from unboundednerfpytorch_amd import grid

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError("library call %s" % name)
    monkeypatch.setattr(grid, "_L", NoCalls())
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        grid.TrainSampleTensoRF.apply(*_cpu_factors(), *_op_args())
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        grid.TrainSampleTensoRF.apply(*_cpu_factors(comp_last=tc.FACTORS), *_op_args())
    # two of the six component-last, four canonical: one layout for all six or none
    with pytest.raises(RuntimeError, match="share one layout"):
        grid.TrainSampleTensoRF.apply(*_cpu_factors(comp_last=('xy_plane', 'z_vec')), *_op_args())
    with pytest.raises(RuntimeError, match="share one layout"):
        grid.TrainSampleTensoRF.apply(*_cpu_factors(comp_last=('xz_plane', 'yz_plane', 'x_vec', 'y_vec')), *_op_args())


def test_fused_tensorf_is_off_by_default_and_gates_can_fuse():
    from unboundednerfpytorch_amd import grid
    from unboundednerfpytorch_amd.train_model import TrainModel
    from unboundednerfpytorch_amd.voxgo_model import DirectContractedVoxGO, DirectVoxGO
    assert TrainModel.fused_tensorf is False
    fake_cuda, fake_cpu = type('T', (), {'is_cuda': True})(), type('T', (), {'is_cuda': False})()
    for density_type in ('TensoRFGrid', 'DenseGrid'):
        m = DirectVoxGO(**tc.model_kwargs('dvgo', density_type))
        assert m.fused_tensorf is False and m._can_fuse(fake_cuda) is False
        m.fused_tensorf = True
        assert m._can_fuse(fake_cuda) is True and m._can_fuse(fake_cpu) is False and m._native_params() is None
        m.fused_forward = False
        assert m._can_fuse(fake_cuda) is False
        m.fused_forward = True
        # an injected lookup: the march would not sample what the model's density returns -- only a TensoRF DENSITY is concerned
        m.density.query_fn = (lambda *a: None) if density_type == 'TensoRFGrid' else m.density.query_fn
        m.k0.query_fn = grid.tensorf_compose
        assert m._can_fuse(fake_cuda) is (density_type == 'DenseGrid')
    c = DirectContractedVoxGO(**tc.model_kwargs('dcvgo', 'TensoRFGrid'))
    assert c._can_fuse(fake_cuda) is False
    c.fused_tensorf = True
    assert c._can_fuse(fake_cuda) is True and c._native_params() is None
