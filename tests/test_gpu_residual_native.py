"""DirectVoxGO's residual-colour rgbnet (rgbnet_direct = False: rgb = sigmoid(rgbnet([k0[:, 3:], view embedding]) + k0[:, :3]),
dvgo.py:384-398) through the native step -- native_step.VoxGOStep with colour 'residual' (ugrid_voxgo_step.colour = 2), opt-in by
`native_residual = True`:

  * the three elementwise leaves alone (ugrid_rgbnet_features_residual, ugrid_residual_logits, ugrid_residual_k0_grad), through
    ctypes on buffers with canary rows, bit for bit against what they replace;
  * the native step against the OP-BY-OP residual step of the same model (TrainSampleVox, GridQuery, FusedRgbnet on
    k0[:, 3:].contiguous(), the strided add, RenderLoss): same kernels, same sizes, same order -- every forward array, loss, mse and
    the rgbnet's gradients bit for bit, grid gradients and short trajectories under the project's bounds for two runs of the same
    scatter (synth.NATIVE_*);
  * the native step against the reference's own model (tests/golden/voxgo_train_dvgo_fine_residual.npz);
  * the sync-free variant, batches with no live ray and with one, and a hipGraph capture."""
import copy
import os

import numpy as np
import pytest
import torch

import synth
from test_gpu_voxgo_train import build, DVGO_BOX, DVGO_CASES

CASE = DVGO_CASES[1]
assert CASE[0] == "dvgo_fine_residual" and CASE[3] == 9 and CASE[4] is False
PER_SAMPLE = ("weights", "raw_alpha", "raw_density", "raw_logits", "ray_id", "step_id", "t")
SENTINEL, GUARD_ROWS = -7.25, 3
# (k0 channels, viewbase_pe): the case's shape, the config's (mlp_in = 36, channel-last k0 with touch bitmaps), the smallest
MODELS = [(9, 4), (12, 4), (4, 0)]


# ---- 1. the leaves ------------------------------------------------------------------------------------------------------------------
def _guarded(rows, cols, dev):
    """[rows, cols] view with GUARD_ROWS canary rows before and after it -> (view, whole buffer)"""
    whole = torch.full((rows + 2 * GUARD_ROWS, cols), SENTINEL, dtype=torch.float32, device=dev)
    return whole[GUARD_ROWS:GUARD_ROWS + rows], whole


def _canaries_intact(whole, rows):
    return bool((whole[:GUARD_ROWS] == SENTINEL).all()) and bool((whole[GUARD_ROWS + rows:] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("C,pe", [(4, 0), (9, 4), (12, 4), (104, 4)], ids=lambda x: str(x))
def test_residual_leaves_equal_what_they_replace(C, pe):
    from unboundednerfpytorch_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    E, F = 3 + 6 * pe, C - 3
    freq = torch.tensor([2.0 ** i for i in range(pe)], device=dev)
    g = torch.Generator().manual_seed(100 * C + pe)
    with _lib.guard(dev):
        st = _lib.stream_of(freq)
        for m in (0, 1, 255, 256, 257, 4099):
            R = max(1, m // 3)
            k0 = torch.randn(m, C, generator=g).to(dev)
            ray_id = torch.sort(torch.randint(0, R, (m,), generator=g)).values.to(dev)
            viewdirs = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(dev)
            k0_back = k0[:, 3:].contiguous()
            ptr = lambda t: _lib.ptr(t) if t.numel() else None
            for with_rows in (True, False):
                # -- features: against ugrid_rgbnet_features on the contiguous copy, in the same launch variant
                want = torch.empty(m, F + E, device=dev)
                rows_w = torch.empty(R, E, device=dev) if with_rows else None
                assert lib.ugrid_rgbnet_features(ptr(k0_back), F, _lib.ptr(viewdirs), R, ptr(freq), pe, ptr(ray_id), m,
                                                 _lib.ptr(rows_w) if with_rows else None, ptr(want), st) == 0
                got, whole = _guarded(m, F + E, dev)
                (rows_g, rows_whole) = _guarded(R, E, dev) if with_rows else (None, None)
                assert lib.ugrid_rgbnet_features_residual(ptr(k0), C, _lib.ptr(viewdirs), R, ptr(freq), pe, ptr(ray_id), m,
                                                          _lib.ptr(rows_g) if with_rows else None, ptr(got), st) == 0
                torch.cuda.synchronize()
                assert torch.equal(got, want), (m, with_rows)
                assert _canaries_intact(whole, m), (m, with_rows)
                if with_rows:
                    assert _canaries_intact(rows_whole, R)
                    if m >= 2 * R:          # the per-ray-rows variant ran: the scratch holds every ray's embedding
                        assert torch.equal(rows_g, rows_w)
                if m:
                    assert torch.equal(got[:, :F], k0_back) and torch.equal(got[:, F:F + 3], viewdirs[ray_id])
            # -- logits += k0[:, :3]
            net = torch.randn(m, 3, generator=g).to(dev)
            logits, whole = _guarded(m, 3, dev)
            logits.copy_(net)
            assert lib.ugrid_residual_logits(ptr(logits), ptr(k0), C, m, st) == 0
            torch.cuda.synchronize()
            assert torch.equal(logits, net + k0[:, :3]), m
            assert _canaries_intact(whole, m), m
            # -- g_k0 = [g_logits | g_feat]
            g_logits, g_feat = torch.randn(m, 3, generator=g).to(dev), torch.randn(m, F, generator=g).to(dev)
            g_k0, whole = _guarded(m, C, dev)
            assert lib.ugrid_residual_k0_grad(ptr(g_logits), ptr(g_feat), C, m, ptr(g_k0), st) == 0
            torch.cuda.synchronize()
            assert torch.equal(g_k0, torch.cat([g_logits, g_feat], -1)), m
            assert _canaries_intact(whole, m), m


# ---- the models ---------------------------------------------------------------------------------------------------------------------
def _build(C, pe, dev):
    """the dvgo_fine_residual case (tests/golden/gen_golden.py) -- or the same grid, rays and densities with another k0 width /
    view embedding"""
    if (C, pe) == (CASE[3], 4):
        return build("dvgo", CASE, dev)
    from unboundednerfpytorch_amd import voxgo_model as vm
    name, seed, G, _, direct, R, dm, ds = CASE
    m = vm.DirectVoxGO(xyz_min=DVGO_BOX[0], xyz_max=DVGO_BOX[1], num_voxels=G ** 3, num_voxels_base=G ** 3, alpha_init=1e-2,
                       fast_color_thres=1e-4, rgbnet_dim=C, rgbnet_direct=False, viewbase_pe=pe, mask_cache_world_size=None)
    o, d, v = [torch.from_numpy(a) for a in synth.rays(seed, R, origin_scale=0.4)]
    params = synth.dvgo_params(seed, [int(x) for x in m.world_size], C, False, viewbase_pe=pe, dens_mean=dm, dens_std=ds)
    sd = m.state_dict()
    with torch.no_grad():
        for k, val in params.items():
            assert tuple(sd[k].shape) == tuple(val.shape), (k, sd[k].shape, val.shape)
            sd[k].copy_(torch.from_numpy(val))
    return m.to(dev), name, [x.to(dev) for x in (o, d, v)], dict(near=0.2, far=6.0, stepsize=0.5, bg=1, render_depth=True), R, seed


def _pair(dev, C=9, pe=4):
    """model A (native_residual), model B (its deep copy on the op-by-op ops), rays, render kwargs, target"""
    m_a, name, (o, d, v), kw, R, seed = _build(C, pe, dev)
    assert m_a.rgbnet is not None and not m_a.rgbnet_direct and m_a.k0.grid.shape[1] == C
    assert tuple(m_a.rgbnet[0].weight.shape) == (128, C + 6 * pe)
    m_a.native_residual = True
    m_b = copy.deepcopy(m_a)
    m_b.native_step = False
    target = torch.from_numpy(synth.uniform(seed + 5, R * 3).reshape(R, 3)).to(dev) * 0.5 + 0.25
    rk = {k: kw[k] for k in kw if k != "render_depth"}
    return m_a, m_b, (o, d, v), rk, target, R


LOSS_CFG = dict(weight_main=1.0, weight_entropy_last=0.01, weight_rgbper=0.01, weight_nearclip=0.0, weight_distortion=0.0)


def _coef(m, rk, R, dev, cfg=LOSS_CFG):
    from unboundednerfpytorch_amd.ops import loss_coefficients
    return loss_coefficients(cfg, R, m.sample_table(rk["stepsize"], dev).numel(), None, 1)


def _is_native(out):
    return out["loss"].grad_fn is not None and type(out["loss"].grad_fn).__name__.startswith("VoxGOStep")


def _grads_close(ga, gb, rgbnet_bound=None):
    """grid gradients: the scatter's atomic adds in an order that varies run to run; the rgbnet's: fixed-order sums, the same bits
    (rgbnet_bound: the sync-free step cuts the same sums into slabs by the capacity instead of the count)"""
    assert sorted(ga) == sorted(gb)
    for k in ga:
        scale = float(gb[k].abs().max())
        if "grid" in k:
            assert scale > 0
            assert float((ga[k] - gb[k]).abs().max()) <= synth.NATIVE_GRID_GRAD_BOUND * scale, (k, float((ga[k] - gb[k]).abs().max()), scale)
        elif rgbnet_bound is None:
            assert torch.equal(ga[k], gb[k]), k
        else:
            assert float((ga[k] - gb[k]).abs().max()) <= rgbnet_bound * (scale + 1e-30), (k, float((ga[k] - gb[k]).abs().max()), scale)


# ---- 2. native = op by op -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C,pe", MODELS, ids=["case_C9", "config_C12", "smallest_C4_pe0"])
def test_native_residual_step_equals_the_op_by_op_step(C, pe):
    """tests/test_gpu_voxgo_train.py::test_native_step_equals_the_op_by_op_step for the residual rgbnet"""
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model
    dev = torch.device("cuda", 0)
    m_a, m_b, (o, d, v), rk, target, R = _pair(dev, C, pe)
    assert bool(m_a.k0.channels_last) == (C % 4 == 0)            # C = 9: the canonical layout; 12 and 4: channel-last + touch bitmaps
    cfg = dict(lrate_density=1e-1, lrate_k0=1e-1, lrate_rgbnet=1e-3, lrate_decay=20, pg_scale=[], tv_every=1, tv_after=0, tv_before=7,
               tv_dense_before=4, weight_tv_density=1e-5, weight_tv_k0=1e-6, skip_zero_grad_fields=['density', 'k0'], **LOSS_CFG)
    coef = _coef(m_a, rk, R, dev)
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
    pack = oa.pop("native")
    assert pack["colour"] == "residual"
    assert set(oa) == set(ob), (sorted(oa), sorted(ob))
    for k in oa:
        if torch.is_tensor(oa[k]):
            assert torch.equal(oa[k].detach(), ob[k].detach()), k
        else:
            assert oa[k] == ob[k], k
    n = oa["weights"].numel()
    assert n > 100 and oa["raw_logits"].shape == (n, 3)
    if (C, pe) == (9, 4):
        assert abs(n - 943) <= 2 and abs(int(oa["ray_id"].unique().numel()) - 104) <= 1          # the golden's survivors and live rays
    assert len(ga) == 8
    _grads_close(ga, gb)
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
    # not the native step's business: no gradient, the attribute off
    with torch.no_grad():
        out = m_a(o, d, v, global_step=1, is_train=True, fused_loss={'target': target, 'coef': coef}, **rk)
    assert out["loss"].grad_fn is None and out["ray_id"].numel() > 0
    m_a.native_residual = False
    assert not _is_native(m_a(o, d, v, global_step=1, is_train=True, fused_loss={'target': target, 'coef': coef}, **rk))


# ---- 3. against the reference's own model ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_native_residual_step_matches_the_reference_model(golden_dir):
    """The reference's DirectVoxGO(rgbnet_direct=False), one training forward (tests/golden/gen_golden.py::gen_voxgo_train).  Its loss
    has a term the fused loss's coefficients cannot express -- 0.05 sum(weights^2) / R, where weight_rgbper weighs
    sum(stop_grad(w) (rgb - target)^2) / R -- so neither the loss nor the gradients of that file are this step's: the forward arrays
    are compared, under the tolerances of test_fused_training_forward_backward_matches_the_reference_model"""
    dev = torch.device("cuda", 0)
    m, name, (o, d, v), kw, R, seed = build("dvgo", CASE, dev)
    m.native_residual = True
    gold = np.load(os.path.join(golden_dir, "voxgo_train_" + name + ".npz"))
    target = torch.from_numpy(gold["target"]).to(dev)
    rk = {k: kw[k] for k in kw if k != "render_depth"}
    coef = _coef(m, rk, R, dev, dict(LOSS_CFG, weight_rgbper=0.0))
    out = m(o, d, v, global_step=1, is_train=True, fused_loss={'target': target, 'coef': coef}, **rk)
    assert _is_native(out)
    out["loss"].backward()
    torch.cuda.synchronize()
    n, n_gold = int(out["weights"].numel()), int(gold["n_kept"])
    assert n_gold == 943 and abs(n - n_gold) <= 2, (n, n_gold)
    if n == n_gold:
        assert np.array_equal(out["ray_id"].cpu().numpy(), gold["ray_id"])
        for k in ("weights", "raw_alpha"):
            np.testing.assert_allclose(out[k].cpu().numpy(), gold[k], rtol=0, atol=2e-5, err_msg=k)
    for k in ("rgb_marched", "alphainv_last"):          # (rgb_marched: the residual colours composited, bg = 1)
        np.testing.assert_allclose(out[k].cpu().numpy(), gold[k], rtol=0, atol=1e-4, err_msg=k)
    for k, q in m.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()) and bool(q.grad.any()), k


# ---- 4. sync-free ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("C,pe", MODELS[:2], ids=["case_C9", "config_C12"])
def test_sync_free_residual_step_equals_the_host_counted_step(C, pe):
    """tests/test_gpu_coarse_native.py::test_sync_free_coarse_step_equals_the_host_counted_step on the residual model: the three leaves
    take their row count through ug_devn like every per-sample kernel"""
    from unboundednerfpytorch_amd import native_step
    dev = torch.device("cuda", 0)
    m, _, (o, d, v), rk, target, R = _pair(dev, C, pe)
    kw = dict(rk, fused_loss={'target': target, 'coef': _coef(m, rk, R, dev)})
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
        # (the rgbnet's gradients as test_sync_free_step_equals_the_host_counted_step compares them: 1e-5 of their largest entry)
        _grads_close(gb, ga, rgbnet_bound=1e-5)
    native_step._TRACKERS.clear()


# ---- 5. no live ray, one live ray -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_miss,n_hit", [(7, 0), (64, 1)], ids=["all_7_miss", "1_of_65_hits"])
def test_native_residual_step_on_batches_with_no_or_one_live_ray(n_miss, n_hit):
    """M2 = 0 (empty per-sample arrays, zero-sized workspaces, the three leaves launch nothing) and one live ray among 65"""
    dev = torch.device("cuda", 0)
    m_a, m_b, (o, d, v), rk, target, R = _pair(dev)
    g = torch.Generator().manual_seed(3)
    away = torch.nn.functional.normalize(torch.rand(n_miss, 3, generator=g) + 0.2, dim=-1)       # from outside the box, away from it
    o2 = torch.cat([3.0 + torch.rand(n_miss, 3, generator=g), o[:n_hit].cpu()]).to(dev)
    d2 = torch.cat([away * 1.5, d[:n_hit].cpu()]).to(dev)
    v2 = torch.nn.functional.normalize(d2, dim=-1)
    n = n_miss + n_hit
    tg = target[:n].contiguous()
    coef = _coef(m_a, rk, n, dev)
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
        _grads_close(ga, gb)


# ---- 6. hipGraph ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_residual_train_step_is_capturable_in_a_hip_graph():
    """tests/test_gpu_voxgo_train.py::test_train_step_is_capturable_in_a_hip_graph on the residual model: one sync-free step captured,
    replayed on two ray sets.  The eager references run on a side stream and only detached copies are kept (see there)."""
    dev = torch.device("cuda", 0)
    m, _, (o, d, v), rk, target, R = _pair(dev)
    kw = dict(rk, fused_loss={'target': target, 'coef': _coef(m, rk, R, dev)})
    o2, d2, v2 = o.flip(0).contiguous(), d.flip(0).contiguous(), v.flip(0).contiguous()
    t2 = target.flip(0).contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    ref = []
    keep = ("loss_mse", "alphainv_last", "rgb_marched") + PER_SAMPLE
    with torch.cuda.stream(side):
        for rays, tg in (((o, d, v), target), ((o2, d2, v2), t2)):
            m.native_sync_free = False
            m.zero_grad(set_to_none=True)
            out = m(*rays, global_step=1, is_train=True, **dict(kw, fused_loss=dict(kw["fused_loss"], target=tg)))
            assert _is_native(out)
            out["loss"].backward()
            ref.append(({k: out[k].detach().clone() for k in keep if k in out}, {k: p.grad.clone() for k, p in m.named_parameters()}))
            del out
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    so, sd, sv, stg = o.clone(), d.clone(), v.clone(), target.clone()          # static inputs of the graph
    m.native_sync_free = {'hints': (0, 0)}
    m.zero_grad(set_to_none=True)
    kwg = dict(kw, fused_loss=dict(kw["fused_loss"], target=stg))
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                      # warm-up on the side stream (allocator pools, lazy module loads)
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            w = m(so, sd, sv, global_step=1, is_train=True, **kwg)
            w["loss"].backward()
            del w
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=True)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        gout = m(so, sd, sv, global_step=1, is_train=True, **kwg)
        gout["loss"].backward()
        ggrads = {k: p.grad for k, p in m.named_parameters()}
    assert gout["native"]["colour"] == "residual"
    for (rays, tg), (oref, gref) in zip((((o, d, v), target), ((o2, d2, v2), t2)), ref):
        so.copy_(rays[0]); sd.copy_(rays[1]); sv.copy_(rays[2]); stg.copy_(tg)
        for p in ggrads.values():
            p.zero_()
        g.replay()
        torch.cuda.synchronize()
        n = oref["weights"].numel()
        assert n > 100 and int(gout["native"]["out"]["n_valid"][1]) == n
        assert torch.equal(gout["loss_mse"], oref["loss_mse"])
        for k in ("alphainv_last", "rgb_marched"):
            assert torch.equal(gout[k], oref[k]), k
        for k in PER_SAMPLE:
            if k in oref:
                assert torch.equal(gout[k][:n], oref[k]), k
        _grads_close(ggrads, gref, rgbnet_bound=1e-5)
