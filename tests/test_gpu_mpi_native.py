"""The native training step of the forward-facing model on the GPU: mpi_model.DirectMPIGO through native_step.VoxGOStep mode 'mpi'
(ugrid_voxgo_step mode 3: ugrid_train_sample_mpi, the compaction with the s table, the canonical k0 lookup, the 3 x 64 rgbnet, the loss
with s given) against the OP-BY-OP step of the same model (native_step = False: grid.TrainSampleVox('mpi'), GridQuery, ops.FusedRgbnet,
ops.RenderLoss -- four autograd nodes), which is what the model did before the native step existed.  The C side runs the same kernels on
the same sizes in the same order, so everything without atomics is compared with torch.equal; the two grid gradients are scatters with
fp32 atomics and are compared under the bounds below.

Shapes: tests/mpi_cases.py MPI_CASES[0] -- 300 rays (no multiple of 64), 47 samples per ray, a 20 x 19 x 24 grid, C = 9 (canonical k0
layout), width 64; edge batches of 3 rays and a 6 x 6 x 256 grid (the deepest shift table, 511 samples per ray)."""
import copy

import numpy as np
import pytest
import torch

import mpi_cases
import synth
from test_mpi_train import build

pytestmark = pytest.mark.gpu

# Bounds that are measurements (tools/native_step_spread.py --cases mpi --reps 50, profiles/mpi/native_step_spread.json: op-by-op vs
# op-by-op and native vs op-by-op at exactly these shapes, 50 repetitions on one MI355X).  The op-by-op vs op-by-op maxima lie within the
# bounds the other models' native-step tests use (tests/synth.py NATIVE_*), so those are used as they are:
#   grid gradients    max |dA - dB| / max |dB|    op vs op 1.26e-7  (native vs op 1.26e-7)    synth.NATIVE_GRID_GRAD_BOUND = 8e-6
#   loss trajectory   max relative difference      op vs op 1.91e-7  (native vs op 1.91e-7)    synth.NATIVE_LOSS_RTOL = 5e-7
#   parameters after the 8 steps: largest difference 0.033 of a learning-rate step in either comparison (bound 0.85), at most 2 entries of
#   a tensor further apart than 2 % of a step (bound max(4, ...))                               synth.assert_same_trajectory
# Forward arrays, loss, mse and the rgbnet's gradients were bit-identical in all 50: torch.equal there.
GRID_GRAD_BOUND = 8e-6
#   loss trajectory   max relative difference       op vs op 0 (native vs op 0)                    synth.NATIVE_LOSS_RTOL = 5e-7
#   parameters after 8 steps                        op vs op 0.0 lr steps (native vs op 0.0)       synth.assert_same_trajectory
GRID_GRAD_BOUND = synth.NATIVE_GRID_GRAD_BOUND
LOSS_RTOL = synth.NATIVE_LOSS_RTOL
LLFF = dict(weight_main=1.0, weight_entropy_last=0.001, weight_rgbper=0.01, weight_nearclip=0.0, weight_distortion=0.01)
PER_SAMPLE = ("weights", "raw_alpha", "raw_logits", "ray_id", "s")
PER_RAY = ("alphainv_last", "rgb_marched")


def setup(dev, rand_bkgd=False):
    """MPI_CASES[0]'s model with the native step switched on EXPLICITLY, its rays, the render kwargs and the fused-loss dict"""
    from unboundednerfpytorch_amd.ops import loss_coefficients
    case = mpi_cases.MPI_CASES[0]
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    m, (o, d, v), kw = build(case, dev)
    m.native_step = True
    target = torch.from_numpy(synth.uniform(seed + 5, R * 3).reshape(R, 3).astype(np.float32)).to(dev) * 0.5 + 0.25
    rk = {k: kw[k] for k in kw if k != "render_depth"}
    if rand_bkgd:
        rk["rand_bkgd"] = True
    coef = loss_coefficients(LLFF, R, m.sample_table(stepsize, dev).numel(), None, 1)
    return m, (o, d, v), rk, {'target': target, 'coef': coef}


def op_by_op_twin(m):
    t = copy.deepcopy(m)
    t.native_step = False
    return t


def forward_backward(m, rays, rk, fl, seed=5):
    m.zero_grad(set_to_none=True)
    torch.manual_seed(seed)
    out = m(*rays, global_step=1, is_train=True, fused_loss=fl, **rk)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {k: (p.grad.clone() if p.grad is not None else None) for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    return out, grads


def is_native(out):
    return out["loss"].grad_fn is not None and type(out["loss"].grad_fn).__name__.startswith("VoxGOStep")


def assert_native_equals_twin(oa, ga, ob, gb, what):
    """the return dicts and gradients of the native step (a) and of the op-by-op step (b) on the same inputs"""
    assert is_native(oa) and not is_native(ob), what
    oa = dict(oa)
    assert torch.equal(oa.pop("loss_mse"), torch.stack([ob["loss"], ob["mse"]]).detach()), what
    oa.pop("native")
    assert set(oa) == set(ob), (what, sorted(oa), sorted(ob))
    assert "raw_density" not in oa and "step_id" not in oa and "t" not in oa
    for k in oa:
        if torch.is_tensor(oa[k]):
            assert oa[k].dtype == ob[k].dtype and torch.equal(oa[k].detach(), ob[k].detach()), (what, k)
        else:
            assert oa[k] == ob[k], (what, k)
    assert sorted(ga) == sorted(gb)
    for k in ga:
        if k != "act_shift.grid" and (ga[k] is None or gb[k] is None):
            # (a batch without samples: autograd may leave a parameter without a gradient where the other step hands out zeros)
            assert oa["weights"].numel() == 0 and all(g is None or not bool(g.any()) for g in (ga[k], gb[k])), (what, k)
        elif k == "act_shift.grid":
            assert ga[k] is None and gb[k] is None, what        # the per-plane shift is not trained
        elif "grid" in k:      # the lookups' scatters add with hardware atomics: the same terms in an order that varies run to run
            scale = float(gb[k].abs().max())
            err = float((ga[k] - gb[k]).abs().max())
            print("%s: grad %s diff / max %.3g" % (what, k, err / (scale + 1e-30)))
            assert err <= GRID_GRAD_BOUND * scale, (what, k, err, scale)
            assert torch.equal(ga[k] != 0, gb[k] != 0), (what, k)          # the voxels MaskedAdam will update
        else:                  # fixed-order sums: the same bits
            assert torch.equal(ga[k], gb[k]), (what, k)


def test_native_step_equals_the_op_by_op_step():
    dev = torch.device("cuda", 0)
    m_a, rays, rk, fl = setup(dev, rand_bkgd=True)
    m_b = op_by_op_twin(m_a)
    oa, ga = forward_backward(m_a, rays, rk, fl)
    ob, gb = forward_backward(m_b, rays, rk, fl)
    assert_native_equals_twin(oa, ga, ob, gb, "mpi_fine")
    assert oa["weights"].numel() > 500 and oa["n_max"] == 47 and oa["s"].dtype == torch.float32
    assert set(oa) - {"native", "loss_mse"} == {"alphainv_last", "weights", "rgb_marched", "raw_alpha", "raw_logits", "ray_id", "n_max", "s",
                                                 "loss", "mse"}
    # not the native step's business: a no-grad forward, the switch
    with torch.no_grad():
        out = m_a(*rays, global_step=1, is_train=True, fused_loss=fl, **rk)
    assert out["loss"].grad_fn is None and "native" not in out and out["ray_id"].numel() > 0


def test_short_training_trajectories_stay_together():
    """8 train_iteration steps of the native and of the op-by-op model through the dense-TV, masked-TV and no-TV phases with llff's loss
    weights and the random background (train_iteration reads the native step's loss_mse); first loss identical, losses and parameters under the atomic-order bounds, the loss goes down"""
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model
    dev = torch.device("cuda", 0)
    m_a, (o, d, v), rk, fl = setup(dev, rand_bkgd=True)
    m_b, fresh_native = op_by_op_twin(m_a), copy.deepcopy(m_a)
    cfg = dict(LLFF, lrate_density=1e-1, lrate_k0=1e-1, lrate_rgbnet=1e-3, lrate_decay=20, pg_scale=[], tv_every=1, tv_after=0, tv_before=7,
               tv_dense_before=4, weight_tv_density=1e-5, weight_tv_k0=1e-6, skip_zero_grad_fields=['density', 'k0'])
    shift0 = m_a.act_shift.grid.detach().clone()
    res = []
    for m in (m_a, m_b):
        torch.manual_seed(11)
        opt = create_optimizer_or_freeze_model(m, cfg, global_step=0)
        losses = [ts.train_iteration(m, opt, o, d, v, fl['target'], cfg, step, rk) for step in range(1, 9)]
        torch.cuda.synchronize()
        res.append((losses, {k: p.detach().clone() for k, p in m.named_parameters()}))
    print("native losses", ["%.6f" % x[0] for x in res[0][0]], "op-by-op", ["%.6f" % x[0] for x in res[1][0]])
    assert res[0][0][0][0] == res[1][0][0][0], (res[0][0][0], res[1][0][0])     # first step: identical parameters, identical loss
    assert abs(res[0][0][0][1] - res[1][0][0][1]) <= 1e-5                        # (psnr: host log10 of the same float32 mse)
    np.testing.assert_allclose(np.array(res[0][0]), np.array(res[1][0]), rtol=LOSS_RTOL)
    synth.assert_same_trajectory(res[0][1], res[1][1])
    assert res[0][0][-1][0] < res[0][0][0][0]
    # the same eight steps with the k0 update started from the native node's mid-backward callback (train_iteration's
    # overlap_k0_update -> pack['k0_grad_ready'], ugrid_voxgo_step_backward_k0 / _density): the same trajectory
    m_c = fresh_native
    torch.manual_seed(11)
    opt = create_optimizer_or_freeze_model(m_c, cfg, global_step=0)
    losses = [ts.train_iteration(m_c, opt, o, d, v, fl['target'], cfg, step, rk, overlap_k0_update=True) for step in range(1, 9)]
    torch.cuda.synchronize()
    assert losses[0][0] == res[1][0][0][0]
    np.testing.assert_allclose(np.array(losses), np.array(res[1][0]), rtol=LOSS_RTOL)
    synth.assert_same_trajectory({k: p.detach().clone() for k, p in m_c.named_parameters()}, res[1][1])
    assert torch.equal(m_a.act_shift.grid, shift0) and m_a.act_shift.grid.grad is None


def test_edge_batches_three_rays_all_misses_and_the_deepest_table():
    from unboundednerfpytorch_amd.mpi_model import DirectMPIGO
    from unboundednerfpytorch_amd.ops import loss_coefficients
    dev = torch.device("cuda", 0)
    m_a, (o, d, v), rk, fl = setup(dev)
    m_b = op_by_op_twin(m_a)
    # R = 3 (less than one block of four waves), ray 1 misses the box entirely
    o3, d3, v3 = o[:3].clone(), d[:3].clone(), v[:3].clone()
    o3[1] = torch.tensor([5.0, 5.0, -1.0], device=dev)
    d3[1] = torch.tensor([0.0, 0.0, 2.0], device=dev)
    fl3 = {'target': fl['target'][:3].contiguous(), 'coef': loss_coefficients(LLFF, 3, 47, None, 1)}
    oa, ga = forward_backward(m_a, (o3, d3, v3), rk, fl3)
    ob, gb = forward_backward(m_b, (o3, d3, v3), rk, fl3)
    assert_native_equals_twin(oa, ga, ob, gb, "three rays")
    assert oa["weights"].numel() > 0 and int((oa["ray_id"] == 1).sum()) == 0 and float(oa["alphainv_last"][1]) == 1.0
    assert torch.equal(oa["rgb_marched"][1], torch.ones(3, device=dev))                  # bg = 1
    # EVERY ray misses: M1 = M2 = 0 -- the loss is the background's, every gradient is zero
    om, dm_ = o3[1:2].expand(3, 3).contiguous(), d3[1:2].expand(3, 3).contiguous()
    oa, ga = forward_backward(m_a, (om, dm_, v3), rk, fl3)
    ob, gb = forward_backward(m_b, (om, dm_, v3), rk, fl3)
    assert_native_equals_twin(oa, ga, ob, gb, "all rays miss")
    assert oa["weights"].numel() == 0 and oa["raw_logits"].shape == (0, 3) and oa["s"].numel() == 0
    assert torch.equal(oa["alphainv_last"], torch.ones(3, device=dev)) and torch.equal(oa["rgb_marched"], torch.ones(3, 3, device=dev))
    # (the mean of 9 squares in float32, summed in another order than torch's: 9 roundings of 2^-24 at the most, < 1e-6 relative)
    assert float(oa["mse"]) == pytest.approx(float(((1.0 - fl3['target']) ** 2).mean()), rel=1e-6) and bool(torch.isfinite(oa["loss"]))
    assert all(g is None or not bool(g.any()) for g in ga.values())
    # mpi_depth = 256 on a 6 x 6 x 256 grid: the deepest shift table the march takes, 511 samples per ray (eight rounds of 64)
    torch.manual_seed(7)
    big = DirectMPIGO(xyz_min=mpi_cases.XYZ_MIN, xyz_max=mpi_cases.XYZ_MAX, num_voxels=256 * 40, mpi_depth=256,
                      fast_color_thres=mpi_cases.fast_color_thres(0.5, 256), rgbnet_dim=9, rgbnet_depth=3, rgbnet_width=64, viewbase_pe=0)
    assert big.world_size.tolist() == [6, 6, 256] and big.n_samples(0.5) == 511
    with torch.no_grad():
        big.density.grid.copy_(torch.randn(big.density.grid.shape) * 1.5 - 1.5)
        big.k0.grid.copy_(torch.randn(big.k0.grid.shape))
    big = big.to(dev)
    big.native_step = True
    twin = op_by_op_twin(big)
    rays = (o[:40].contiguous(), d[:40].contiguous(), v[:40].contiguous())
    flb = {'target': fl['target'][:40].contiguous(), 'coef': loss_coefficients(LLFF, 40, 511, None, 1)}
    kb = dict(near=0, far=1, stepsize=0.5, bg=1)
    oa, ga = forward_backward(big, rays, kb, flb)
    ob, gb = forward_backward(twin, rays, kb, flb)
    assert_native_equals_twin(oa, ga, ob, gb, "mpi_depth 256")
    assert oa["n_max"] == 511 and oa["weights"].numel() > 500 and float(oa["s"].max()) > 0.9


def assert_sync_free_equals(out, grads, oref, gref, what):
    """a sync-free (capacity-sized) result against the host-counted one: per-ray arrays and the written rows bit-equal, grid gradients
    within the atomic bound, the rgbnet's within 1e-5 of their largest entry (the same sums cut into slabs by the capacity)"""
    n = oref["weights"].numel()
    nv = out["native"]["out"]["n_valid"].tolist()
    assert nv[1] == n and nv[0] >= n, (what, nv, n)
    assert out["weights"].numel() > n, what          # capacity-sized
    assert torch.equal(out["loss_mse"], oref["loss_mse"]), what
    for k in PER_RAY:
        assert torch.equal(out[k], oref[k]), (what, k)
    for k in PER_SAMPLE:
        assert torch.equal(out[k][:n], oref[k]), (what, k)
    for k in gref:
        if gref[k] is None:
            assert grads[k] is None, (what, k)
            continue
        scale = float(gref[k].abs().max()) + 1e-30
        bound = GRID_GRAD_BOUND if "grid" in k else 1e-5
        err = float((gref[k] - grads[k]).abs().max())
        assert err <= bound * scale, (what, k, err, scale)


def test_sync_free_step_equals_the_host_counted_step():
    """native_sync_free (ugrid_voxgo_step.sync_free: no host read, capacity-sized arrays, the counts on the device) against the
    host-counted native step: with no hint, with hints far BELOW the counts (the kernels must loop) and with the tracker's own hints
    on a second call; then a stage-2 capacity below the count -- rows clamped, the overflow reported by the tracker one step late"""
    from unboundednerfpytorch_amd import native_step
    dev = torch.device("cuda", 0)
    m, rays, rk, fl = setup(dev)
    native_step._TRACKERS.clear()
    m.native_sync_free = False
    oref, gref = forward_backward(m, rays, rk, fl)
    assert is_native(oref)
    oref = {k: (x.detach().clone() if torch.is_tensor(x) else x) for k, x in oref.items() if k != "native"}
    n = oref["weights"].numel()
    assert n > 500
    for sf in (True, {'hints': (64, 16)}, True):
        m.native_sync_free = sf
        out, grads = forward_backward(m, rays, rk, fl)
        assert is_native(out)
        assert_sync_free_equals(out, grads, oref, gref, "sync_free=%r" % (sf,))
    # the tracker learnt the counts from the earlier calls: the last call's grids followed them
    tr = [t for key, t in native_step._TRACKERS.items() if key[1] == 'mpi']
    assert len(tr) == 1 and tr[0].poll()[1] == n
    # a caller-chosen stage-2 capacity below the count
    cap = n // 2
    native_step._TRACKERS.clear()
    m.native_sync_free = {'capacity': cap}
    m.zero_grad(set_to_none=True)
    out = m(*rays, global_step=1, is_train=True, fused_loss=fl, **rk)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert out["weights"].numel() == cap and out["s"].numel() == cap and int(out["native"]["out"]["n_valid"][1]) == n
    assert bool(torch.isfinite(out["loss"])) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.requires_grad)
    assert bool((out["ray_id"][1:] >= out["ray_id"][:-1]).all()) and int(out["ray_id"].max()) < 300      # the kept prefix is ray-major
    for k in PER_SAMPLE:                                  # ... and is the host-counted step's prefix
        assert torch.equal(out[k], oref[k][:cap]), k
    with pytest.raises(RuntimeError, match="raise the capacity"):
        m(*rays, global_step=1, is_train=True, fused_loss=fl, **rk)
    native_step._TRACKERS.clear()


def test_train_step_is_capturable_in_a_hip_graph():
    """The sync-free step -- forward, loss and the whole backward -- captured ONCE in a hipGraph and replayed on a second ray set (same
    buffers): loss_mse, the per-ray arrays and the written rows of the per-sample arrays bit-equal to the eager host-counted step on
    those rays; gradients within the bounds of the sync-free test.  Discipline of tests/test_gpu_voxgo_train.py's twin: eager
    references and the warm-up on a side stream, only detached copies kept, no reseeding inside the capture."""
    dev = torch.device("cuda", 0)
    m, (o, d, v), rk, fl = setup(dev)
    o2, d2, v2, tg2 = o.flip(0).contiguous(), d.flip(0).contiguous(), v.flip(0).contiguous(), fl['target'].flip(0).contiguous()
    sets = (((o, d, v), fl['target']), ((o2, d2, v2), tg2))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    ref = []
    keep = ("loss_mse",) + PER_RAY + PER_SAMPLE
    with torch.cuda.stream(side):
        for rays, tg in sets:
            m.native_sync_free = False
            m.zero_grad(set_to_none=True)
            out = m(*rays, global_step=1, is_train=True, fused_loss=dict(fl, target=tg), **rk)
            assert is_native(out)
            out["loss"].backward()
            ref.append(({k: out[k].detach().clone() for k in keep}, {k: (p.grad.clone() if p.grad is not None else None)
                                                                      for k, p in m.named_parameters()}))
            del out
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    # static inputs of the graph
    so, sd, sv, stg = o.clone(), d.clone(), v.clone(), fl['target'].clone()
    m.native_sync_free = {'hints': (0, 0)}
    m.zero_grad(set_to_none=True)
    flg = dict(fl, target=stg)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up on the side stream (allocator pools, lazy module loads)
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            w = m(so, sd, sv, global_step=1, is_train=True, fused_loss=flg, **rk)
            w["loss"].backward()
            del w
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = m(so, sd, sv, global_step=1, is_train=True, fused_loss=flg, **rk)
        gout["loss"].backward()
        ggrads = {k: p.grad for k, p in m.named_parameters()}
    assert ggrads["act_shift.grid"] is None
    for (rays, tg), (oref, gref) in zip(sets, ref):
        so.copy_(rays[0]); sd.copy_(rays[1]); sv.copy_(rays[2]); stg.copy_(tg)
        for p in ggrads.values():
            if p is not None:
                p.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert oref["weights"].numel() > 500
        assert_sync_free_equals(gout, ggrads, oref, gref, "replay")
    assert not torch.equal(ref[0][0]["rgb_marched"], ref[1][0]["rgb_marched"])          # the second ray set is another batch
