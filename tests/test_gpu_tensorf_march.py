"""The fused sampling march over a TensoRF density (grid.TrainSampleTensoRF: k_train_march_tensorf + the dense march's compaction and
backward + the factorised lookup's backward over the stage-1 points) and TrainModel.fused_tensorf on the MI355X:

  1. the density the march stores is the stand-alone query kernel's, bit for bit, at the points it stores (both models, both layouts);
  2. DirectVoxGO with fused_tensorf = True equals the op-by-op chain in everything the sampling decides (both layouts, and the
     dense-density + TensoRF-k0 model, which takes grid.TrainSampleVox);
  3. DirectContractedVoxGO, inf and l2 norm: the same samples, values to the 2e-6 of the dense-grid test (the chain's `norm` is an ulp off);
  4. the reference's own models (tests/golden/tensorf_models.npz) under the bound of tests/test_gpu_tensorf_model.py;
  5. rays without samples, batches without samples;
  6. the reference's 40 training steps (tests/golden/tensorf_train.npz) across a scale_volume_grid.

Set-up of 1-3 and 5: the box of tensorf_cases (three different axis lengths; the contracted model's separating box), 40^3 voxels
(DirectVoxGO: world 44 x 35 x 40, the longest ray has 142 slots; the contracted model: 40^3 and a sample table of 134 -- three trips of
the march's 64-sample loop either way), n_comp 3 / n_comp_xy 2, 70 rays (17 full blocks of four waves and a ragged one), a solid block
of the mask cache cleared."""
import os

import numpy as np
import pytest
import torch

import tensorf_cases as tc
import test_gpu_tensorf_model as tm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = tm.GOLD
NVOX, N_RAYS, THRES = 40 ** 3, 70, 1e-4
BLOCK = (slice(10, 20), slice(8, 16), slice(12, 30))          # mask-cache voxels set False
KW = {'dvgo': dict(tc.RENDER_KW), 'dcvgo': dict(stepsize=0.5, bg=1)}
# (model seed, ray seed, density scale) per configuration: chosen on the CPU with the reference's own models so that the preconditions
# the tests assert hold -- a ray that ends below 1e-3 transmittance, rays without samples, no alpha or weight at the threshold
SETUP = {('dvgo', 'TensoRFGrid'): (41, 42, 12.0), ('dvgo', 'DenseGrid'): (43, 44, 5.0), ('dcvgo', 'TensoRFGrid'): (45, 46, 12.0)}


# Test 3 compares with a chain whose points are an ulp off (torch's `norm`), so what it measures is (an ulp of position) x (the
# density's gradient): its 2e-6 is the dense-grid test's number and was taken on that test's fields, the roughest of which
# (dcvgo_fine_inf: N(1, 5) voxels, 14^3) has an RMS gradient of 44 per unit length.  This file's factors x 12 give 102.5 per unit at
# 40^3 (both by central differences over 200 k points on the CPU); the field is quadratic in the factor, so x 12 * sqrt(44 / 102.5) =
# 7.87 matches that roughness.  Test 3 alone uses it, rounded down; at x 12 its largest weight difference is 2.25e-6.
DCVGO_CHAIN_SCALE = 7.8


def build_model(kind, density_type='TensoRFGrid', comp_last=False, norm='inf', device=DEV, scale=None):
    """the model of this file's set-up; the same logical parameters in either factor layout (the draws do not depend on the storage)"""
    from unboundednerfpytorch_amd import grid
    from unboundednerfpytorch_amd.voxgo_model import DirectContractedVoxGO, DirectVoxGO
    seed = SETUP[(kind, density_type)][0]
    scale = SETUP[(kind, density_type)][2] if scale is None else scale
    tensorf = density_type == 'TensoRFGrid'
    kw = dict(xyz_min=tc.XYZ_MIN, xyz_max=tc.XYZ_MAX, num_voxels=NVOX, num_voxels_base=NVOX, alpha_init=1e-2, fast_color_thres=THRES,
              density_type=density_type, density_config=dict(n_comp=3, n_comp_xy=2) if tensorf else {}, k0_type='TensoRFGrid',
              k0_config=dict(n_comp=5), rgbnet_dim=12, rgbnet_width=32)
    kw.update(dict(rgbnet_direct=True) if kind == 'dvgo' else dict(contracted_norm=norm))
    torch.manual_seed(seed)
    old = grid.TensoRFGrid.component_last
    grid.TensoRFGrid.component_last = bool(comp_last)
    try:
        m = (DirectVoxGO if kind == 'dvgo' else DirectContractedVoxGO)(**kw)
    finally:
        grid.TensoRFGrid.component_last = old
    for g in (m.density, m.k0):
        if isinstance(g, grid.TensoRFGrid):
            g.component_last = bool(comp_last)          # (what a later scale_volume_grid stores)
    with torch.no_grad():
        if tensorf:          # tensorf_cases.structure_density, with this file's factor
            for p in m.density.parameters():
                p.mul_(scale)
        else:
            m.density.grid.copy_(torch.randn(m.density.grid.shape, generator=torch.Generator().manual_seed(3)) * scale)
        m.mask_cache.mask[BLOCK] = False
    return m.to(device)


def make_rays(kind, density_type='TensoRFGrid', device=DEV):
    """70 rays of tensorf_cases.model_rays: the first five with origins x 6, and (DirectVoxGO) one that looks away from the box"""
    o, d, v = tc.model_rays(N_RAYS, SETUP[(kind, density_type)][1], kind)
    o[:5] *= 6.0
    if kind == 'dvgo':
        d[5] = o[5]
        v[5] = d[5] / np.linalg.norm(d[5])
    return [torch.from_numpy(a).to(device) for a in (o, d, v)]


def spied_forward(m, o, d, v, kw):
    """the model's forward with its fused sampling call recorded: (out, {'t', 'cfg', 'out': the op's nine outputs, 'calls'})"""
    rec = {'calls': 0}
    orig = m._fused_sample

    def spy(rays_o, rays_d, t, cfg):
        rec.update(t=t, cfg=cfg, out=orig(rays_o, rays_d, t, cfg), calls=rec['calls'] + 1)
        return rec['out']
    m._fused_sample = spy
    try:
        return m(o, d, v, **kw), rec
    finally:
        del m._fused_sample


def graph_ops(t):
    """the names of the autograd nodes below a tensor"""
    seen, names, todo = set(), set(), [t.grad_fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        names.add(type(n).__name__)
        todo.extend(f for f, _ in n.next_functions)
    return names


def assert_op_ran(t, density_type):
    """the fused sampling op of this density type, and not the other one, produced `t`"""
    names = graph_ops(t)
    want, other = "TrainSampleTensoRFBackward", "TrainSampleVoxBackward"
    if density_type != 'TensoRFGrid':
        want, other = other, want
    assert want in names and other not in names, sorted(names)


@torch.no_grad()
def composed_chain(m, kind, o, d, stepsize, near=None, **_):
    """The op-by-op sampling of the models' composed forwards (voxgo_model.py, the `else` branches), restated with everything it
    decides kept: the surviving samples and, for the threshold preconditions, EVERY alpha behind the mask cache and every weight
    behind the alpha threshold"""
    from unboundednerfpytorch_amd import ops, ub360_utils_cuda
    N = o.shape[0]
    interval = stepsize * m.voxel_size_ratio
    if kind == 'dvgo':
        pts, ray_id, step_id = m.sample_ray(rays_o=o, rays_d=d, near=near, far=None, stepsize=stepsize)
    else:
        pts, inner, t = m.sample_ray(ori_rays_o=o, ori_rays_d=d, stepsize=stepsize)
        n_max = t.numel()
        ray_id = torch.arange(N, device=o.device).view(-1, 1).expand(N, n_max)
        step_id = torch.arange(n_max, device=o.device).view(1, -1).expand(N, n_max)
        keep = inner.clone()
        dist = (pts[:, 1:] - pts[:, :-1]).norm(dim=-1)
        keep[:, 1:] |= ub360_utils_cuda.cumdist_thres(dist.contiguous(), (2 + 2 * m.bg_len) / m.world_len * stepsize * 0.95)
        pts, ray_id, step_id = pts[keep], ray_id[keep], step_id[keep]
    k = m.mask_cache(pts)
    pts, ray_id, step_id = pts[k], ray_id[k], step_id[k]
    n_masked = pts.shape[0]
    density = m.density(pts)
    alpha_all = m.activate_density(density, interval)
    k = alpha_all > m.fast_color_thres
    pts, ray_id, step_id, density, alpha = pts[k], ray_id[k], step_id[k], density[k], alpha_all[k]
    weights_all, ainv = ops.Alphas2Weights.apply(alpha, ray_id, N)
    k = weights_all > m.fast_color_thres
    return dict(pts=pts[k], ray_id=ray_id[k], step_id=step_id[k], density=density[k], alpha=alpha[k], weights=weights_all[k],
                alphainv_last=ainv, alpha_all=alpha_all, weights_all=weights_all, n_masked=n_masked, n_stage1=int(alpha.numel()))


def loss_of(out, target):
    """mse + the background entropy + a weight term: gradient reaches the density through rgb_marched, alphainv_last and the weights"""
    loss = torch.nn.functional.mse_loss(out["rgb_marched"], target)
    p = out["alphainv_last"].clamp(1e-6, 1 - 1e-6)
    loss = loss + 0.01 * (-(p * torch.log(p) + (1 - p) * torch.log(1 - p))).mean()
    return loss + 0.05 * (out["weights"] * out["weights"]).sum() / target.shape[0]


def fused_and_composed(m, o, d, v, kw):
    """forward + backward with fused_tensorf True and False in one process, the library rgbnet on both sides (only the sampling
    differs) -> {flag: (out, gradients, the recorded sampling call or None)}"""
    m.fused_rgbnet = False
    target = tc.train_target(v)
    res = {}
    for fused in (True, False):
        m.fused_tensorf = fused
        m.zero_grad(set_to_none=True)
        out, rec = spied_forward(m, o, d, v, kw)
        loss_of(out, target).backward()
        res[fused] = (out, {k: p.grad.clone() for k, p in m.named_parameters()}, rec if rec['calls'] else None)
    assert res[True][2] is not None and res[True][2]['calls'] == 1 and res[False][2] is None
    return res


# ------------------------------------------------------------------------------------------------ 1. leaf identity, op level
@pytest.mark.parametrize("comp_last", [False, True], ids=["canonical", "comp_last"])
@pytest.mark.parametrize("kind", ["dvgo", "dcvgo"])
def test_march_stores_the_density_of_the_query_kernel_bit_for_bit(kind, comp_last):
    from unboundednerfpytorch_amd import _lib, grid
    m = build_model(kind, comp_last=comp_last)
    m.fused_tensorf = True
    assert all(_lib.is_comp_last(p) == comp_last for p in m.density.factors())
    o, d, v = make_rays(kind)
    with torch.no_grad():
        _, rec = spied_forward(m, o, d, v, KW[kind])          # (the arguments the model hands to the op)
    factors = tuple(p.detach() for p in m.density.factors())
    call = lambda: grid.TrainSampleTensoRF.apply(*factors, o.contiguous(), d.contiguous(), rec['t'], m.xyz_min, m.xyz_max, m.mask_cache.mask,
                                                 rec['cfg'])
    first, second = call(), call()
    pts2, dens2, alpha2, w2, ainv, ray2, step2, tt2, inner2 = first
    slots = rec['t'].numel() if kind == 'dcvgo' else rec['cfg']['slots']
    print("%s comp_last=%d: %d stage-2 samples, %d slots per ray, largest step id %d" % (kind, comp_last, w2.numel(), slots, int(step2.max())))
    assert w2.numel() > 500 and slots > 128 and int(step2.max()) >= 64          # the march's sample loop makes three trips
    assert torch.equal(grid.tensorf_query(factors, None, pts2, m.xyz_min, m.xyz_max), dens2)
    assert torch.equal(m.activate_density(dens2, KW[kind]['stepsize'] * m.voxel_size_ratio), alpha2)          # ops.Raw2Alpha
    assert int(step2.min()) >= 0 and int(step2.max()) < slots
    assert bool((ray2[1:] >= ray2[:-1]).all()) and int(ray2.min()) >= 0 and int(ray2.max()) < N_RAYS
    key = ray2 * slots + step2
    assert bool((key[1:] > key[:-1]).all())                                    # ray-major, near to far, no sample twice
    assert bool((w2 > THRES).all()) and bool((alpha2 > THRES).all()) and ainv.shape == (N_RAYS,)
    assert inner2.dtype == torch.bool and (kind == 'dcvgo' or bool(inner2.all()))
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    for a, b in zip(first, rec['out']):                                          # what the model got is what the op gives
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ 2. DirectVoxGO: fused == composed
@pytest.mark.parametrize("density_type,comp_last", [("TensoRFGrid", False), ("TensoRFGrid", True), ("DenseGrid", False)],
                         ids=["tensorf_canonical", "tensorf_comp_last", "dense_density_tensorf_k0"])
def test_dvgo_fused_sampling_equals_the_op_by_op_chain(density_type, comp_last):
    m = build_model('dvgo', density_type, comp_last)
    o, d, v = make_rays('dvgo', density_type)
    kw = KW['dvgo']
    # the preconditions, on the composed side
    m.fused_tensorf = False
    assert not m._can_fuse(o)
    ch = composed_chain(m, 'dvgo', o, d, **kw)
    per_ray = torch.bincount(ch['ray_id'], minlength=N_RAYS)
    print("composed: %d behind the mask cache, %d stage-1, %d stage-2 samples; largest step id %d; %d rays below 1e-3, %d rays without a sample" % (
        ch['n_masked'], ch['n_stage1'], ch['ray_id'].numel(), int(ch['step_id'].max()), int((ch['alphainv_last'] < 1e-3).sum()),
        int((per_ray == 0).sum())))
    assert int(ch['step_id'].max()) >= 64
    assert int((ch['alphainv_last'] < 1e-3).sum()) >= 1
    assert int((per_ray == 0).sum()) >= 1
    assert ch['ray_id'].numel() > 500
    res = fused_and_composed(m, o, d, v, kw)
    (a, ga, rec), (b, gb, _) = res[True], res[False]
    assert_op_ran(a['weights'], density_type)
    assert not graph_ops(b['weights']) & {"TrainSampleTensoRFBackward", "TrainSampleVoxBackward"}
    assert torch.equal(b['ray_id'], ch['ray_id']) and torch.equal(b['weights'], ch['weights'])          # the chain above is the model's
    assert torch.equal(rec['out'][6], ch['step_id'].long())
    for k in ("ray_id", "weights", "raw_alpha", "alphainv_last"):
        assert torch.equal(a[k], b[k]), k
    assert float((a['rgb_marched'] - b['rgb_marched']).detach().abs().max()) <= 1e-6
    assert sorted(ga) == sorted(gb)
    for k in ga:
        scale = float(gb[k].abs().max()) + 1e-20
        err = float((ga[k] - gb[k]).abs().max())
        print("grad %s: |fused - composed| / max = %.2e" % (k, err / scale))
        assert err <= 1e-4 * scale, (k, err / scale)


# ------------------------------------------------------------------------------------------------ 3. DirectContractedVoxGO
@pytest.mark.parametrize("norm", ["inf", "l2"])
def test_dcvgo_fused_sampling_equals_the_op_by_op_chain(norm):
    """the composed chain's `norm` (ray directions; the l2 norm of the points) is an ulp off on this torch build, as the dense-grid test
    of tests/test_gpu_voxgo_train.py notes: same samples -- no alpha or weight of the chain sits within 1e-5 of the threshold --, values to
    2e-6, on a density as rough as that test's (DCVGO_CHAIN_SCALE above).  Exactness is test 1's."""
    m = build_model('dcvgo', norm=norm, scale=DCVGO_CHAIN_SCALE)
    o, d, v = make_rays('dcvgo')
    kw = KW['dcvgo']
    m.fused_tensorf = False
    ch = composed_chain(m, 'dcvgo', o, d, **kw)
    for name in ('alpha_all', 'weights_all'):
        margin = float((ch[name] / THRES - 1).abs().min())
        print("%s: %s closest to the threshold at %.3e (relative)" % (norm, name, margin))
        assert margin > 1e-5, (name, margin)
    assert ch['ray_id'].numel() > 500 and int(ch['step_id'].max()) >= 64
    res = fused_and_composed(m, o, d, v, kw)
    (a, ga, _), (b, gb, _) = res[True], res[False]
    assert_op_ran(a['weights'], 'TensoRFGrid')
    assert torch.equal(b['ray_id'], ch['ray_id']) and torch.equal(b['step_id'], ch['step_id'])
    for k in ("ray_id", "step_id"):
        assert torch.equal(a[k], b[k]), k
    for k in ("weights", "raw_alpha", "alphainv_last"):
        err = float((a[k] - b[k]).detach().abs().max())
        print("%s %s: |fused - composed| = %.2e" % (norm, k, err))
        assert err <= 2e-6, (k, err)


# ------------------------------------------------------------------------------------------------ 4. the reference's own models
@pytest.mark.parametrize("case", tc.MODEL_CASES, ids=[c[0] for c in tc.MODEL_CASES])
def test_fused_model_matches_the_reference_model(case):
    """tests/test_gpu_tensorf_model.py's comparison with the reference's own model (fixture: float32 and float64 on the CPU), taken
    through the fused sampling: the kept-sample list exactly, every output and parameter gradient under that file's `within`"""
    name, kind, density_type, seed, ray_seed = case
    z = np.load(os.path.join(GOLD, "tensorf_models.npz"))
    state = {k[len(name) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "/sd/")}
    m = tm.build(kind, seed, density_type, state=state)
    m.fused_tensorf = True
    o, d, v = tm.rays(64, ray_seed, kind)
    assert m._can_fuse(o)
    out = m(o, d, v, **KW[kind])
    assert_op_ran(out['weights'], density_type)
    out['rgb_marched'].sum().backward()
    ref_id = torch.from_numpy(z[name + "/ray_id"]).to(DEV)
    assert ref_id.numel() > 1000 and torch.equal(out['ray_id'], ref_id)
    for k in tc.MODEL_KEYS:
        tm.within(name, k, out[k], z["%s/out/%s/32" % (name, k)], z["%s/out/%s/64" % (name, k)])
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(k.split("/")[2] for k in z.files if k.startswith(name + "/grad/") and k.endswith("/64"))
    for k, p in params.items():
        assert p.grad is not None, k
        tm.within(name, "grad " + k, p.grad, z["%s/grad/%s/32" % (name, k)], z["%s/grad/%s/64" % (name, k)])


# ------------------------------------------------------------------------------------------------ 5. edges
def test_a_ray_that_misses_has_no_sample_and_shows_the_background():
    m = build_model('dvgo')
    m.fused_tensorf = True
    o, d, v = [x[3:8].contiguous() for x in make_rays('dvgo')]          # R = 5; ray 2 of them looks away from the box
    out = m(o, d, v, **KW['dvgo'])
    assert_op_ran(out['weights'], 'TensoRFGrid')
    per_ray = torch.bincount(out['ray_id'], minlength=5)
    assert int(per_ray[2]) == 0 and int(per_ray.sum()) > 0
    assert float(out['alphainv_last'][2]) == 1.0
    assert torch.equal(out['rgb_marched'][2], torch.ones(3, device=DEV))          # bg = 1
    out['rgb_marched'].sum().backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_a_batch_without_samples_gives_empty_lists_and_zero_gradients_without_a_launch(monkeypatch):
    from unboundednerfpytorch_amd import grid
    m = build_model('dvgo', comp_last=True)
    m.fused_tensorf = True
    o, d, v = make_rays('dvgo')
    d = o.clone()                                                          # every ray looks away from the box
    with torch.no_grad():
        out, rec = spied_forward(m, o, d, v, KW['dvgo'])
    assert all(x.shape[0] == 0 for i, x in enumerate(rec['out']) if i != 4)
    assert out['ray_id'].numel() == 0 and out['weights'].numel() == 0
    assert torch.equal(out['rgb_marched'], torch.ones(N_RAYS, 3, device=DEV))          # bg = 1: the background everywhere
    factors = m.density.factors()
    outs = grid.TrainSampleTensoRF.apply(*factors, o, d, None, m.xyz_min, m.xyz_max, m.mask_cache.mask, rec['cfg'])
    assert outs[3].numel() == 0 and torch.equal(outs[4], torch.ones(N_RAYS, device=DEV))
    called = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            called.append(name)
            return getattr(self._lib, name)
    monkeypatch.setattr(grid, "_L", Spy(grid._L))
    (outs[3].sum() + outs[4].sum() + outs[1].sum()).backward()
    assert called == [], called
    for p in factors:
        assert p.grad is not None and p.grad.stride() == p.stride() and not bool(p.grad.any())


# ------------------------------------------------------------------------------------------------ 6. training
def test_training_through_the_fused_march_matches_the_reference_run():
    """the 40 steps of tests/test_gpu_tensorf_model.py's `trained` fixture with fused_tensorf = True: train_iteration's fused tail
    behind the fused sampling, the TV window, and a scale_volume_grid at step 20 -- the op reads the factors of the moment"""
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model
    z = np.load(os.path.join(GOLD, "tensorf_train.npz"))
    state = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    m = tm.build('dvgo', tc.TRAIN_SEED, width=128, nvox=tc.TRAIN_VOXELS // 2, state=state)
    m.fused_tensorf = True
    o, d, v = tm.rays(256, tc.TRAIN_RAY_SEED)
    target = tc.train_target(v)
    opt = create_optimizer_or_freeze_model(m, tc.TRAIN_CFG, global_step=0)
    calls, shapes, orig = [], set(), m._fused_sample

    def spy(rays_o, rays_d, t, cfg):
        calls.append(1)
        shapes.add(tuple(m.density.xy_plane.shape))
        return orig(rays_o, rays_d, t, cfg)
    m._fused_sample = spy
    losses, psnrs = [], []
    for step in range(1, tc.TRAIN_STEPS + 1):
        opt = ts.maybe_scale_grids(m, opt, tc.TRAIN_CFG, dict(num_voxels=tc.TRAIN_VOXELS), step)
        loss, psnr = ts.train_iteration(m, opt, o, d, v, target, tc.TRAIN_CFG, step, tm.RK)
        losses.append(loss)
        psnrs.append(psnr)
    del m._fused_sample
    assert len(calls) == tc.TRAIN_STEPS and len(shapes) == 2          # every step sampled through the op, at both resolutions
    p32, p64 = float(z["psnr/32"][-1]), float(z["psnr/64"][-1])
    margin = max(4 * abs(p32 - p64), 0.01)
    print("loss %.5f -> %.5f, psnr %.3f -> %.4f dB; reference fp32 %.4f, fp64 %.4f dB, margin %.3f dB" % (
        losses[0], losses[-1], psnrs[0], psnrs[-1], p32, p64, margin))
    assert abs(psnrs[0] - float(z["psnr/32"][0])) < 1e-3
    assert all(np.isfinite(losses)) and int(m.num_voxels) == tc.TRAIN_VOXELS and m.density.xy_plane.shape[2] == int(m.world_size[0])
    assert abs(psnrs[-1] - p32) <= margin, (psnrs[-1], p32, p64)
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
    for k, p in m.named_parameters():
        assert bool(torch.isfinite(p).all()), k
