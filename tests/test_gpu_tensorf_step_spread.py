"""How far apart are two runs of the SAME op-by-op `fused_tensorf` training step of a TensoRF model on the MI355X?

The factorised lookup's backward adds with fp32 atomics (csrc/ugrid_tensorf.hip), so two runs of one step agree in their factor
gradients to rounding only.  A native step over TensoRF grids (not built) will have to be compared with this step, and
its bound has to come from what this step shows against ITSELF.  This file is the set-up of that comparison and the floor, for the
six configurations such a step has to cover: DirectVoxGO TensoRF / TensoRF in both factor layouts, dense density + TensoRF k0,
TensoRF density + dense k0 (a combination no other test runs through the fused sampling), DirectContractedVoxGO inf and l2.

Set-up: tests/test_gpu_tensorf_march.py's (40^3 voxels, density n_comp 3 / 2, k0 n_comp 5, rgbnet 12 -> 32, 70 rays, a cleared mask
block), the fused loss of tensorf_cases.TRAIN_CFG.

Measured with tools/tensorf_step_spread.py, 100 repetitions per configuration (profiles/tensorf/step_spread.json): the largest
max|dA - dB| / max|dB| between two runs is 6.3e-7 for planes (8.8e-7 in an earlier run of the same 100 repetitions), 4.5e-7 for
vectors, 3.3e-7 for f_vec, 8.3e-8 for a dense grid; forward arrays, loss, mse and the rgbnet's gradients were bit-identical in every
repetition, and so was the set of zero entries of every gradient.  4 x the largest figure is below synth.NATIVE_GRID_GRAD_BOUND =
8e-6, the bound of the dense models' native-step tests, which is therefore asserted here as it is."""
import pytest
import torch

import synth
import tensorf_cases as tc
import test_gpu_tensorf_march as tmarch
from test_gpu_tensorf_march import KW, build_model, make_rays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# name: kind, density type, component-last factors, contracted norm, dense k0
STEP_CASES = {"dvgo_tt_canonical": ("dvgo", "TensoRFGrid", False, "inf", False), "dvgo_tt_comp_last": ("dvgo", "TensoRFGrid", True, "inf", False),
              "dvgo_dense_density_tensorf_k0": ("dvgo", "DenseGrid", False, "inf", False),
              "dvgo_tensorf_density_dense_k0": ("dvgo", "TensoRFGrid", False, "inf", True),
              "dcvgo_inf": ("dcvgo", "TensoRFGrid", False, "inf", False), "dcvgo_l2": ("dcvgo", "TensoRFGrid", False, "l2", False)}


def kind_of(name):
    """the tensor kind of a parameter name, or None for the fixed-order (rgbnet) gradients"""
    if name.endswith("f_vec"):
        return "f_vec"
    if name.endswith("_plane"):
        return "plane"
    if name.endswith("_vec"):
        return "vector"
    return "grid" if name.endswith(".grid") else None


def with_dense_k0(m):
    """the (host) model with its TensoRF k0 replaced by a dense one of the same channels, channel-last as the models build it: the
    TensoRF-density + dense-k0 combination, which the set-up of tests/test_gpu_tensorf_march.py does not build"""
    m.k0 = m._make_typed_grid('DenseGrid', m.k0_dim, {}, True)
    with torch.no_grad():
        m.k0.grid.copy_(torch.randn(m.k0.grid.shape, generator=torch.Generator().manual_seed(48)) * 0.3)
    m.k0_type, m.k0_config = 'DenseGrid', {}
    return m


def setup_case(name):
    """-> model (fused_tensorf on), (o, d, v), render kwargs with the fused loss of tensorf_cases.TRAIN_CFG"""
    from unboundednerfpytorch_amd import ops
    kind, density_type, comp_last, norm, dense_k0 = STEP_CASES[name]
    m = build_model(kind, density_type, comp_last, norm, device="cpu")
    if dense_k0:
        with_dense_k0(m)
    m = m.to(DEV)
    m.fused_tensorf = True
    rays = make_rays(kind, density_type)
    coef = ops.loss_coefficients(tc.TRAIN_CFG, rays[0].shape[0], m.sample_table(KW[kind]['stepsize'], DEV).numel(), None, 1)
    kw = dict(KW[kind], fused_loss={'target': tc.train_target(rays[2]), 'coef': coef})
    return m, rays, kw


def run_step(m, rays, kw):
    """one forward + backward of the model's training step -> (the return dict, {name: gradient clone}); complete on return"""
    m.zero_grad(set_to_none=True)
    out = m(*rays, global_step=1, is_train=True, **kw)
    out["loss"].backward()
    torch.cuda.synchronize()
    return out, {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_two_runs_of_the_op_by_op_step_agree(name):
    m, rays, kw = setup_case(name)
    kind, density_type, _, _, dense_k0 = STEP_CASES[name]
    oa, ga = run_step(m, rays, kw)
    ob, gb = run_step(m, rays, kw)
    names = tmarch.graph_ops(oa["loss"])
    assert ("TrainSampleTensoRFBackward" if density_type == "TensoRFGrid" else "TrainSampleVoxBackward") in names, sorted(names)
    assert ("TensoRFQueryBackward" in names) == (not dense_k0), sorted(names)          # (the k0 lookup's op; a dense k0 has GridQuery's)
    assert oa["weights"].numel() > 500 and bool(torch.isfinite(oa["loss"]))
    for k, x in ob.items():
        if torch.is_tensor(x):
            assert torch.equal(oa[k].detach(), x.detach()), k          # every forward array, loss and mse: bit for bit
    assert sorted(ga) == sorted(gb) and {kind_of(k) for k in ga} >= {None, "plane", "vector"}
    for k in gb:
        scale, err = float(gb[k].abs().max()), float((ga[k] - gb[k]).abs().max())
        print("%s grad %s [%s]: %.3e of max %.3e" % (name, k, kind_of(k), err / scale if scale else err, scale))
        assert scale > 0 and ga[k].stride() == gb[k].stride() == dict(m.named_parameters())[k].stride(), k
        if kind_of(k) is None:
            assert torch.equal(ga[k], gb[k]), k                       # fixed summation order
        else:
            assert err <= synth.NATIVE_GRID_GRAD_BOUND * scale, (k, err, scale)
            # the masked Adam skips exactly-zero gradients: the set of zero entries must not depend on the order of the atomics
            assert torch.equal(ga[k] == 0, gb[k] == 0), k
