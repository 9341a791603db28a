"""The coarse stage of DirectVoxGO / DirectContractedVoxGO (no rgbnet, 3-channel k0: rgb = sigmoid(k0)) through the native step --
native_step.VoxGOStep with colour 'none' (ugrid_voxgo_step.colour = 1), opt-in by `native_coarse = True` -- against the OP-BY-OP
coarse step of the same model (TrainSampleVox, GridQuery, RenderLoss; already pinned on the reference's own forward + backward by
tests/test_gpu_voxgo_train.py: voxgo_train_dvgo_coarse.npz, voxgo_train_dcvgo_coarse_l2.npz).  Same kernels, same sizes, same
order: every forward array, the loss and the mse bit for bit; grid gradients and short trajectories under the project's measured
bounds for two runs of the same scatter (synth.NATIVE_*, profiles/r06/native_step_spread.json)."""
import copy

import numpy as np
import pytest
import torch

import synth
from test_gpu_voxgo_train import build, DVGO_CASES

COARSE = [("dvgo", DVGO_CASES[2]), ("dcvgo", synth.DCVGO_CASES[1])]
assert COARSE[0][1][0] == "dvgo_coarse" and COARSE[1][1][0] == "dcvgo_coarse_l2"
PER_SAMPLE = ("weights", "raw_alpha", "raw_density", "raw_logits", "ray_id", "step_id", "t")


def _pair(kind, case, dev):
    """model A (native_coarse), model B (its deep copy on the op-by-op ops), rays, render kwargs, target"""
    m_a, name, (o, d, v), kw, R, seed = build(kind, case, dev)
    assert m_a.rgbnet is None and m_a.k0.grid.shape[1] == 3
    m_a.native_coarse = True
    m_b = copy.deepcopy(m_a)
    m_b.native_step = False
    target = torch.from_numpy(synth.uniform(seed + 5, R * 3).reshape(R, 3)).to(dev) * 0.5 + 0.25
    rk = {k: kw[k] for k in kw if k != "render_depth"}
    return m_a, m_b, (o, d, v), rk, target, R


def _coef(m, kind, rk, R, dev):
    from unboundednerfpytorch_amd.ops import loss_coefficients
    cfg = dict(weight_main=1.0, weight_entropy_last=0.01, weight_rgbper=0.01, weight_nearclip=0.0,
               weight_distortion=0.01 if kind == "dcvgo" else 0.0)
    return loss_coefficients(cfg, R, m.sample_table(rk["stepsize"], dev).numel(), None, 1)


def _is_native(out):
    return out["loss"].grad_fn is not None and type(out["loss"].grad_fn).__name__.startswith("VoxGOStep")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,case", COARSE, ids=[c[0] for _, c in COARSE])
def test_native_coarse_step_equals_the_op_by_op_step(kind, case):
    """tests/test_gpu_voxgo_train.py::test_native_step_equals_the_op_by_op_step for the coarse stage"""
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model
    dev = torch.device("cuda", 0)
    m_a, m_b, (o, d, v), rk, target, R = _pair(kind, case, dev)
    if kind == "dcvgo":
        rk["rand_bkgd"] = True
    cfg = dict(lrate_density=1e-1, lrate_k0=1e-1, lrate_rgbnet=1e-3, lrate_decay=20, pg_scale=[], weight_main=1.0, weight_entropy_last=0.01,
               weight_rgbper=0.01, weight_nearclip=0.0, weight_distortion=0.01 if kind == "dcvgo" else 0.0, tv_every=1, tv_after=0,
               tv_before=7, tv_dense_before=4, weight_tv_density=1e-5, weight_tv_k0=1e-6, skip_zero_grad_fields=['density', 'k0'])
    coef = _coef(m_a, kind, rk, R, dev)
    outs = []
    for m in (m_a, m_b):
        torch.manual_seed(5)
        out = m(o, d, v, global_step=1, is_train=True, fused_loss={'target': target, 'coef': coef}, **rk)
        out["loss"].backward()
        outs.append((out, {k: p.grad.clone() for k, p in m.named_parameters()}))
        m.zero_grad(set_to_none=True)
    (oa, ga), (ob, gb) = outs
    assert _is_native(oa), type(oa["loss"].grad_fn)
    assert not _is_native(ob)
    assert torch.equal(oa.pop("loss_mse"), torch.stack([ob["loss"], ob["mse"]]).detach())
    oa.pop("native")
    assert set(oa) == set(ob), (sorted(oa), sorted(ob))
    for k in oa:
        if torch.is_tensor(oa[k]):
            assert torch.equal(oa[k].detach(), ob[k].detach()), k
        else:
            assert oa[k] == ob[k], k
    assert oa["weights"].numel() > 100 and oa["raw_logits"].shape == (oa["weights"].numel(), 3)
    assert sorted(ga) == ["density.grid", "k0.grid"]
    for k in ga:          # the lookups' scatter adds with hardware atomics: the same terms in an order that varies run to run
        scale = float(gb[k].abs().max())
        assert scale > 0
        assert float((ga[k] - gb[k]).abs().max()) <= synth.NATIVE_GRID_GRAD_BOUND * scale, (k, float((ga[k] - gb[k]).abs().max()), scale)
    # eight training steps through the dense-TV, masked-TV and no-TV phases
    res = []
    for m in (m_a, m_b):
        torch.manual_seed(11)
        opt = create_optimizer_or_freeze_model(m, cfg, global_step=0)
        losses = [ts.train_iteration(m, opt, o, d, v, target, cfg, step, rk) for step in range(1, 9)]
        torch.cuda.synchronize()
        res.append((losses, {k: p.detach().clone() for k, p in m.named_parameters()}))
    assert res[0][0][0][0] == res[1][0][0][0], (res[0][0][0], res[1][0][0])    # first step: identical parameters, identical loss
    assert abs(res[0][0][0][1] - res[1][0][0][1]) <= 1e-5                       # (psnr: host log10 of the same float32 mse)
    np.testing.assert_allclose(np.array(res[0][0]), np.array(res[1][0]), rtol=synth.NATIVE_LOSS_RTOL)
    synth.assert_same_trajectory(res[0][1], res[1][1])
    # not the native step's business: no gradient, a frozen grid, the attribute off
    with torch.no_grad():
        out = m_a(o, d, v, global_step=1, is_train=True, fused_loss={'target': target, 'coef': coef}, **rk)
    assert out["loss"].grad_fn is None and out["ray_id"].numel() > 0
    m_a.native_coarse = False
    assert not _is_native(m_a(o, d, v, global_step=1, is_train=True, fused_loss={'target': target, 'coef': coef}, **rk))


@pytest.mark.gpu
def test_sync_free_coarse_step_equals_the_host_counted_step():
    """native_sync_free = True on the coarse stage (capacity-sized arrays, counts on the device; the k0 lookup and its scatter take
    their row count through ug_devn like every per-sample kernel): the first n_valid rows of every per-sample array, the per-ray
    arrays, loss and mse equal the host-counted native step's; grid gradients within the scatter's atomic-order bound"""
    from unboundednerfpytorch_amd import native_step
    dev = torch.device("cuda", 0)
    kind, case = COARSE[0]
    m, _, (o, d, v), rk, target, R = _pair(kind, case, dev)
    kw = dict(rk, fused_loss={'target': target, 'coef': _coef(m, kind, rk, R, dev)})
    native_step._TRACKERS.clear()
    res = []
    for sf in (False, True, {'hints': (100, 50)}, True):
        m.native_sync_free = sf
        m.zero_grad(set_to_none=True)
        out = m(o, d, v, global_step=1, is_train=True, **kw)
        assert _is_native(out)
        out["loss"].backward()
        torch.cuda.synchronize()
        res.append((out, {k: p.grad.clone() for k, p in m.named_parameters()}))
    oa, ga = res[0]
    n = oa["weights"].numel()
    assert n > 100
    for ob, gb in res[1:]:
        nv = ob["native"]["out"]["n_valid"].tolist()
        assert nv[1] == n and nv[0] >= n, (nv, n)
        assert ob["weights"].numel() > n          # capacity-sized
        assert torch.equal(ob["loss_mse"], oa["loss_mse"])
        assert torch.equal(ob["loss"].detach(), oa["loss"].detach()) and torch.equal(ob["mse"], oa["mse"])
        for k in ("alphainv_last", "rgb_marched"):
            assert torch.equal(ob[k], oa[k]), k
        for k in PER_SAMPLE:
            if k in oa:             # (DirectVoxGO's return dict has no raw_density / step_id / t, like the reference's)
                assert torch.equal(ob[k][:n], oa[k]), k
        for k in ga:
            scale = float(ga[k].abs().max())
            assert float((ga[k] - gb[k]).abs().max()) <= synth.NATIVE_GRID_GRAD_BOUND * scale, (k, float((ga[k] - gb[k]).abs().max()), scale)
    native_step._TRACKERS.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("n_miss,n_hit", [(7, 0), (64, 1)], ids=["all_7_miss", "1_of_65_hits"])
def test_native_coarse_step_on_batches_with_no_or_one_live_ray(n_miss, n_hit):
    """M2 = 0 (no sample survives anywhere: empty per-sample arrays, zero-sized workspaces) and one live ray among 65 (a second,
    nearly empty wave): a finite loss equal to the op-by-op step's, and grid gradients that are exactly zero where nothing survives"""
    dev = torch.device("cuda", 0)
    kind, case = COARSE[0]
    m_a, m_b, (o, d, v), rk, target, R = _pair(kind, case, dev)
    # rays that leave from outside the box, away from it
    g = torch.Generator().manual_seed(3)
    away = torch.nn.functional.normalize(torch.rand(n_miss, 3, generator=g) + 0.2, dim=-1)
    o2 = torch.cat([3.0 + torch.rand(n_miss, 3, generator=g), o[:n_hit].cpu()]).to(dev)
    d2 = torch.cat([away * 1.5, d[:n_hit].cpu()]).to(dev)
    v2 = torch.nn.functional.normalize(d2, dim=-1)
    n = n_miss + n_hit
    tg = target[:n].contiguous()
    coef = _coef(m_a, kind, rk, n, dev)
    outs = []
    for m in (m_a, m_b):
        out = m(o2, d2, v2, global_step=1, is_train=True, fused_loss={'target': tg, 'coef': coef}, **rk)
        out["loss"].backward()
        torch.cuda.synchronize()
        outs.append((out, {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}))
    (oa, ga), (ob, gb) = outs
    assert _is_native(oa) and not _is_native(ob)
    assert bool(torch.isfinite(oa["loss"])) and torch.equal(oa["loss"].detach(), ob["loss"].detach()) and torch.equal(oa["mse"], ob["mse"])
    for k in ("alphainv_last", "rgb_marched", "weights", "raw_alpha", "raw_logits", "ray_id"):
        assert torch.equal(oa[k], ob[k].detach()), k
    assert bool((oa["alphainv_last"][:n_miss] == 1).all())
    if n_hit == 0:
        assert oa["weights"].numel() == 0 and oa["raw_logits"].shape == (0, 3)
        for k in ga:
            assert not bool(ga[k].any()) and not bool(gb[k].any()), k
    else:
        assert oa["weights"].numel() > 0 and bool((oa["ray_id"] == n_miss).all())
        for k in ga:
            scale = float(gb[k].abs().max())
            assert scale > 0 and float((ga[k] - gb[k]).abs().max()) <= synth.NATIVE_GRID_GRAD_BOUND * scale, k
