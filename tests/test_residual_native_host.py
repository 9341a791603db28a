"""DirectVoxGO's residual-colour rgbnet (rgbnet_direct = False: rgb = sigmoid(rgbnet([k0[:, 3:], view embedding]) + k0[:, :3]),
dvgo.py:384-398) on the native step -- HOST side, on the CPU: which configurations select native_step.VoxGOStep with colour
'residual' (opt-in: TrainModel.native_residual), the unchanged struct and ABI version, the limits of ugrid_voxgo_step.colour = 2
checked before anything touches the device, and its two workspace sizes against the formula in include/ugrid_hip.h.  The
kernels' results are tests/test_gpu_residual_native.py's business."""
import ctypes

import pytest
import torch

from test_coarse_native_host import FG, KW
from test_mpi_native_host import model as mpi_model

INVALID, NOT_SUPPORTED = 1, 801          # hipErrorInvalidValue, hipErrorNotSupported


def _residual(**kw):
    from unboundednerfpytorch_amd import voxgo_model as vm
    return vm.DirectVoxGO(**dict(dict(rgbnet_dim=9, rgbnet_direct=False), **kw), **KW)


def test_the_residual_rgbnet_takes_the_native_step_only_when_asked():
    m = _residual()
    assert m.native_residual is False and m.rgbnet is not None and not m.rgbnet_direct
    assert m._native_params() is None                              # the default: the op-by-op ops
    m.native_residual = True
    p = m._native_params()
    assert p is not None and len(p) == 8
    assert p[0] is m.density.grid and p[1] is m.k0.grid and p[1].shape[1] == 9
    assert tuple(p[2].shape) == (128, 9 - 3 + 3 + 6 * 4) and p[2] is m.rgbnet[0].weight and p[7] is m.rgbnet[-1].bias
    # still not the native step's business: a frozen parameter, no gradient, native_step off
    for q in (m.density.grid, m.k0.grid, m.rgbnet[0].weight, m.rgbnet[-1].bias):
        q.requires_grad_(False)
        assert m._native_params() is None
        q.requires_grad_(True)
    with torch.no_grad():
        assert m._native_params() is None
    assert m._native_params() is not None
    m.native_step = False
    assert m._native_params() is None
    m.native_step = True
    m.native_residual = False
    assert m._native_params() is None


def test_native_residual_refuses_what_the_direct_case_refuses():
    deep = _residual(rgbnet_depth=4)                               # not the default 3-layer net
    deep.native_residual = True
    assert deep._native_params() is None
    m = _residual()
    m.native_residual = True
    assert m._native_params() is not None
    m.k0.query_fn = lambda *a: None                                # an injected query function
    assert m._native_params() is None
    m.k0.query_fn = None
    m.density.query_fn = lambda *a: None
    assert m._native_params() is None
    m.density.query_fn = None
    assert m._native_params() is not None
    m.fused_rgbnet = False
    assert m._native_params() is None
    small = _residual(rgbnet_dim=4)                                # the smallest: one feature channel behind the diffuse three
    small.native_residual = True
    assert len(small._native_params()) == 8 and tuple(small.rgbnet[0].weight.shape) == (128, 4 + 6 * 4)


def test_native_residual_leaves_the_other_configurations_alone():
    from unboundednerfpytorch_amd import voxgo_model as vm
    from unboundednerfpytorch_amd.fourier_model import FourierGridModel
    direct = vm.DirectVoxGO(rgbnet_dim=12, rgbnet_direct=True, **KW)
    before = direct._native_params()
    direct.native_residual = True
    after = direct._native_params()
    assert len(before) == len(after) == 8 and all(a is b for a, b in zip(before, after))
    coarse = vm.DirectVoxGO(rgbnet_dim=0, **KW)
    coarse.native_residual = True
    assert coarse._native_params() is None                        # (the coarse stage has its own attribute)
    coarse.native_coarse = True
    assert coarse._native_params()[2:] == [None] * 6
    for m in (vm.DirectContractedVoxGO(rgbnet_dim=12, **KW), FourierGridModel(rgbnet_dim=12, **FG), mpi_model(rgbnet_dim=9)):
        assert m.rgbnet is not None
        before = m._native_params()
        m.native_residual = True
        after = m._native_params()
        assert before is not None and len(before) == len(after) == 8 and all(a is b for a, b in zip(before, after)), type(m)
        assert m._residual_colour() is False and m._native_residual_ok is False


def _step(colour, C, pe, width, M1=1000, M2=130, R=8192):
    from unboundednerfpytorch_amd import _lib
    s = _lib.VoxgoStep()
    s.mode, s.P, s.kP, s.slots = 0, 1, 1, 40
    s.colour, s.C, s.pe, s.width, s.n_rays, s.M1, s.M2 = colour, C, pe, width, R, M1, M2
    return s


def test_colour_2_keeps_the_struct_and_the_abi_version():
    from unboundednerfpytorch_amd import _lib
    lib = _lib.load()
    assert ctypes.sizeof(_lib.VoxgoStep) == lib.ugrid_voxgo_step_sizeof() == 696
    names = [n for n, _ in _lib.VoxgoStep._fields_]
    assert names[:4] == ["mode", "k0_channels_last", "P", "freq_num"] and names[-2:] == ["plane_shift", "mpi_depth"]
    i = names.index("colour")
    assert names[i - 1] == "sync_free" and names[i + 1] == "ws"
    assert _lib.VoxgoStep.colour.offset == _lib.VoxgoStep.sync_free.offset + 4 and _lib.VoxgoStep.colour.size == 4
    assert lib.ugrid_abi_version() == 3
    for fn in ("ugrid_rgbnet_features_residual", "ugrid_residual_logits", "ugrid_residual_k0_grad"):
        assert fn in _lib._SIGNATURES and hasattr(lib, fn)


def test_colour_2_limits_are_checked_before_the_device_is_touched():
    from unboundednerfpytorch_amd import _lib
    lib = _lib.load()
    fwd = lambda s: lib.ugrid_voxgo_step_forward(ctypes.addressof(s), None)
    assert fwd(_step(2, 3, 4, 128)) == INVALID                   # no feature channel behind the diffuse three
    assert fwd(_step(2, 0, 4, 128)) == INVALID
    assert fwd(_step(3, 9, 4, 128)) == INVALID                   # no such colour
    assert fwd(_step(2, 9, 4, 0)) == NOT_SUPPORTED               # the rgbnet's limits: 1 <= width <= 128, C + 6 pe <= 128
    assert fwd(_step(2, 9, 4, 129)) == NOT_SUPPORTED
    assert fwd(_step(2, 105, 4, 128)) == NOT_SUPPORTED
    assert fwd(_step(0, 102, 4, 128)) == NOT_SUPPORTED           # (colour 0's own limit, C + 3 + 6 pe <= 128, is where it was)
    # an admissible colour-2 step gets past the checks: with samples but no workspace it is refused one line later, still on the host
    ok = _step(2, 104, 4, 128)
    assert fwd(ok) == INVALID and lib.ugrid_voxgo_step_ws_floats(ctypes.addressof(ok)) > 0
    # the leaves: C < 4, a negative count, NULL with m > 0; m == 0 launches nothing
    assert lib.ugrid_rgbnet_features_residual(None, 3, None, 1, None, 0, None, 0, None, None, None) == INVALID
    assert lib.ugrid_rgbnet_features_residual(None, 4, None, 1, None, 0, None, -1, None, None, None) == INVALID
    assert lib.ugrid_rgbnet_features_residual(None, 4, None, 1, None, 0, None, 5, None, None, None) == INVALID
    assert lib.ugrid_rgbnet_features_residual(None, 4, None, 1, None, 0, None, 0, None, None, None) == 0
    assert lib.ugrid_residual_logits(None, None, 3, 0, None) == INVALID
    assert lib.ugrid_residual_logits(None, None, 4, -1, None) == INVALID
    assert lib.ugrid_residual_logits(None, None, 4, 5, None) == INVALID
    assert lib.ugrid_residual_logits(None, None, 4, 0, None) == 0
    assert lib.ugrid_residual_k0_grad(None, None, 3, 0, None, None) == INVALID
    assert lib.ugrid_residual_k0_grad(None, None, 4, -1, None, None) == INVALID
    assert lib.ugrid_residual_k0_grad(None, None, 4, 5, None, None) == INVALID
    assert lib.ugrid_residual_k0_grad(None, None, 4, 0, None, None) == 0


@pytest.mark.parametrize("C,pe,width,M1,M2,R", [(9, 4, 128, 1000, 130, 8192), (12, 4, 128, 70001, 4099, 120), (4, 0, 64, 64, 64, 1),
                                                (104, 4, 128, 5, 0, 7)])
def test_colour_2_workspaces_follow_the_formula_of_the_header(C, pe, width, M1, M2, R):
    """include/ugrid_hip.h, ugrid_voxgo_step.colour: al(n) = n rounded up to 64 floats, E = 3 + 6 pe, K = C + 6 pe"""
    from unboundednerfpytorch_amd import _lib
    lib = _lib.load()
    al = lambda n: (n + 63) & ~63
    E, K = 3 + 6 * pe, C + 6 * pe
    s = _step(2, C, pe, width, M1, M2, R)
    scratch = int(lib.ugrid_rgbnet_train_scratch_floats(M2))
    assert lib.ugrid_voxgo_step_ws_floats(ctypes.addressof(s)) == \
        al(3 * M1) + 4 * al(M1) + al(3 * M2) + al(M2 * C) + al(M2 * K) + 2 * al(M2 * width) + al(R * E)
    assert lib.ugrid_voxgo_step_bwd_ws_floats(ctypes.addressof(s)) == \
        al(3 * M2) + 2 * al(M2) + al(R) + al(M2 * C) + al(M1) + al(scratch) + al(M2 * (C - 3))
    # against colour 0 at the same shape: the rgbnet's input is 3 columns narrower, the backward holds the input gradient apart
    d = _step(0, C, pe, width, M1, M2, R)
    if C + E <= 128:
        assert lib.ugrid_voxgo_step_ws_floats(ctypes.addressof(d)) - lib.ugrid_voxgo_step_ws_floats(ctypes.addressof(s)) == \
            al(M2 * (K + 3)) - al(M2 * K)
    assert lib.ugrid_voxgo_step_bwd_ws_floats(ctypes.addressof(s)) - lib.ugrid_voxgo_step_bwd_ws_floats(ctypes.addressof(d)) == al(M2 * (C - 3))


def _apply(m, w0):
    from unboundednerfpytorch_amd import native_step
    lin = [m.rgbnet[0], m.rgbnet[2][0], m.rgbnet[3]]
    return native_step.VoxGOStep.apply(m.density.grid, m.k0.grid, w0, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias,
                                       {'colour': 'residual', 'mode': 'dvgo', 'cfg': {}, 'rays_o': torch.zeros(2, 3), 'rays_d': torch.ones(2, 3),
                                        'viewdirs': torch.ones(2, 3), 'viewfreq': m.viewfreq, 'target': torch.zeros(2, 3)})


def test_voxgo_step_refuses_a_wrong_residual_shape_before_any_launch():
    from unboundednerfpytorch_amd import native_step, voxgo_model as vm
    m = _residual()
    with pytest.raises(RuntimeError, match=r"colour 'residual': w0 must be \[W, C\+6pe\] = \[W, 33\]"):
        _apply(m, torch.zeros(128, 9 + 3 + 24))                  # a first layer of the direct width
    three = vm.DirectVoxGO(rgbnet_dim=3, rgbnet_direct=True, **KW)
    with pytest.raises(RuntimeError, match="colour 'residual' takes a k0 grid .* at least 4 channels"):
        _apply(three, three.rgbnet[0].weight)
    with pytest.raises(RuntimeError, match="colour must be"):
        native_step.VoxGOStep.apply(m.density.grid, m.k0.grid, None, None, None, None, None, None,
                                    {'colour': 'diffuse', 'mode': 'dvgo', 'cfg': {}, 'rays_o': torch.zeros(2, 3), 'rays_d': torch.ones(2, 3),
                                     'target': torch.zeros(2, 3)})
