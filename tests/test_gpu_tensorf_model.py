"""DirectVoxGO / DirectContractedVoxGO with TensoRF grids on the MI355X against the REFERENCE's own models (fixtures written by
tests/golden/gen_tensorf_golden.py on the CPU, float32 and float64): the composed training forward and every parameter gradient on
64 rays, a 40-step training run through train_step.train_iteration (TV window, one scale_volume_grid) against the reference's own
40 steps, and the renderers' from_tensorf_checkpoint (bake, then the fused march + shade kernels) against the training forward."""
import os

import numpy as np
import pytest
import torch

import tensorf_cases as tc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RK = dict(tc.RENDER_KW)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rays(n, seed, kind='dvgo'):
    return [torch.from_numpy(a).to(DEV) for a in tc.model_rays(n, seed, kind)]


def build(kind, seed, density_type='TensoRFGrid', width=32, nvox=12 ** 3, state=None):
    """this package's model with the constructor arguments of tensorf_cases.model_kwargs; state: the reference's state dict"""
    from unboundednerfpytorch_amd.voxgo_model import DirectContractedVoxGO, DirectVoxGO
    torch.manual_seed(seed)
    m = (DirectVoxGO if kind == 'dvgo' else DirectContractedVoxGO)(**tc.model_kwargs(kind, density_type, width, nvox))
    if state is None:
        tc.structure_density(m, density_type)
    else:
        m.load_state_dict(state, strict=True)
    return m.to(DEV)


def within(name, key, got, v32, v64):
    """|hip - fp64| <= 4 x max(the reference's own |fp32 - fp64| of this tensor, 2^-24 x its largest magnitude) -- the floor is half
    an ulp of the largest element, as in tests/test_gpu_tensorf.py (a tensor of three elements can sit below it by chance)"""
    err, scale = float(np.abs(v32.astype(np.float64) - v64).max()), float(np.abs(v64).max())
    eff = max(err, 2.0 ** -24 * scale)
    d = float(np.abs(got.detach().double().cpu().numpy() - v64).max())
    print("%s %s: |hip - fp64| = %.3e, yardstick %.3e (ratio %.2f), scale %.3e" % (name, key, d, err, d / eff if eff else 0.0, scale))
    assert err <= 1e-5 * scale, (name, key, err, scale)          # the yardstick itself is tight
    assert d <= tc.BOUND_FACTOR * eff, (name, key, d, err, scale)


@pytest.mark.parametrize("case", tc.MODEL_CASES, ids=[c[0] for c in tc.MODEL_CASES])
def test_model_forward_and_gradients_match_the_reference_model(case):
    """the reference's own model on the CPU (fixture) against this package's model with the same state dict on the same 64 rays:
    the kept-sample list exactly (the generator asserts that no alpha or weight lies within 1e-5 of fast_color_thres), per-sample and
    per-ray values and every parameter gradient of rgb_marched.sum() under the bound of `within`"""
    name, kind, density_type, seed, ray_seed = case
    z = np.load(os.path.join(GOLD, "tensorf_models.npz"))
    state = {k[len(name) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "/sd/")}
    m = build(kind, seed, density_type, state=state)
    o, d, v = rays(64, ray_seed, kind)
    out = m(o, d, v, **(RK if kind == 'dvgo' else dict(stepsize=0.5, bg=1)))
    out['rgb_marched'].sum().backward()
    ref_id = torch.from_numpy(z[name + "/ray_id"]).to(DEV)
    assert ref_id.numel() > 1000 and torch.equal(out['ray_id'], ref_id)
    for k in tc.MODEL_KEYS:
        within(name, k, out[k], z["%s/out/%s/32" % (name, k)], z["%s/out/%s/64" % (name, k)])
    params = dict(m.named_parameters())
    assert sorted(params) == sorted(k.split("/")[2] for k in z.files if k.startswith(name + "/grad/") and k.endswith("/64"))
    for k, p in params.items():
        assert p.grad is not None, k
        within(name, "grad " + k, p.grad, z["%s/grad/%s/32" % (name, k)], z["%s/grad/%s/64" % (name, k)])


@pytest.fixture(scope="module")
def trained():
    """40 train_iteration steps of a TensoRF DirectVoxGO from the reference's own initial state on the reference's rays and target:
    TV on for the first 20 steps, one scale_volume_grid at step 20 -> (model, losses, psnrs, rays, target)"""
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model
    z = np.load(os.path.join(GOLD, "tensorf_train.npz"))
    state = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    m = build('dvgo', tc.TRAIN_SEED, width=128, nvox=tc.TRAIN_VOXELS // 2, state=state)
    o, d, v = rays(256, tc.TRAIN_RAY_SEED)
    target = tc.train_target(v)
    opt = create_optimizer_or_freeze_model(m, tc.TRAIN_CFG, global_step=0)
    losses, psnrs = [], []
    for step in range(1, tc.TRAIN_STEPS + 1):
        opt = ts.maybe_scale_grids(m, opt, tc.TRAIN_CFG, dict(num_voxels=tc.TRAIN_VOXELS), step)
        loss, psnr = ts.train_iteration(m, opt, o, d, v, target, tc.TRAIN_CFG, step, RK)
        losses.append(loss)
        psnrs.append(psnr)
    return m, losses, psnrs, (o, d, v), target


def test_short_training_run_matches_the_reference_run(trained):
    """the loss halves, and the final PSNR on the training rays lies within 4 x |PSNR of the reference in fp32 - in fp64| (floor
    0.01 dB, the spread README.md documents for training parity) of the reference's own 40 steps"""
    m, losses, psnrs, _, _ = trained
    z = np.load(os.path.join(GOLD, "tensorf_train.npz"))
    p32, p64 = float(z["psnr/32"][-1]), float(z["psnr/64"][-1])
    margin = max(4 * abs(p32 - p64), 0.01)
    print("loss %.5f -> %.5f, psnr %.3f -> %.4f dB; reference fp32 %.4f, fp64 %.4f dB, margin %.3f dB" % (
        losses[0], losses[-1], psnrs[0], psnrs[-1], p32, p64, margin))
    assert abs(psnrs[0] - float(z["psnr/32"][0])) < 1e-3            # the same start
    assert all(np.isfinite(losses)) and int(m.num_voxels) == tc.TRAIN_VOXELS and m.k0.xy_plane.shape[2] == int(m.world_size[0])
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
    assert abs(psnrs[-1] - p32) <= margin, (psnrs[-1], p32, p64)
    for k, p in m.named_parameters():
        assert bool(torch.isfinite(p).all()), k


def _same_as_model(got, want, n_rays):
    """the bound of tests/test_dvgo.py's fused-vs-composed test: no ray beyond 3e-4, at most two beyond 1e-4 (threshold flips)"""
    bad = torch.zeros(n_rays, dtype=torch.bool, device=DEV)
    for k in ('rgb_marched', 'alphainv_last'):
        e = (got[k] - want[k]).abs()
        e = e.amax(dim=1) if e.dim() == 2 else e
        bad |= e > 1e-4
        assert float(e.max()) < 3e-4, (k, float(e.max()))
    assert int(bad.sum()) <= 2, int(bad.sum())


def test_renderer_from_tensorf_checkpoint_equals_the_training_model(trained, tmp_path):
    """the checkpoint of the 40-step run above (act_shift lowered by decay_after_scale at the pg_scale step) through
    DirectVoxGORenderer.from_tensorf_checkpoint: fused kernels on the baked grids against the training model's forward, 256 rays"""
    from unboundednerfpytorch_amd import train_utils
    from unboundednerfpytorch_amd.dvgo_render import DirectVoxGORenderer
    from unboundednerfpytorch_amd.masked_adam import MaskedAdam
    m, _, _, (o, d, v), _ = trained
    path = str(tmp_path / "fine_last.tar")
    train_utils.save_checkpoint(path, m, MaskedAdam([{'params': list(m.parameters()), 'lr': 0.1, 'skip_zero_grad': False}]), 40)
    ck = torch.load(path, map_location='cpu', weights_only=False)
    assert 'k0.f_vec' in ck['model_state_dict'] and 'density.grid' not in ck['model_state_dict']
    rend = DirectVoxGORenderer.from_tensorf_checkpoint(ck, DEV)
    assert rend.fused_supported()
    assert tuple(rend.s['k0_grid'].shape) == (1, 12) + tuple(int(x) for x in m.world_size) and rend.s['k0_grid'].is_contiguous()
    assert float(rend.s['act_shift']) == float(m.act_shift)
    got = rend.render_rays(o, d, v, **RK)
    with torch.no_grad():
        want = m(o, d, v, **RK)
    assert float((want['alphainv_last'] < 0.99).float().mean()) > 0.2
    _same_as_model(got, want, o.shape[0])
    with pytest.raises(RuntimeError, match=r"needs \d+ bytes .* 4096 bytes are free"):
        DirectVoxGORenderer.from_tensorf_checkpoint(ck, DEV, mem_get_info=lambda dev: (4096, 1 << 30))


def test_contracted_renderer_from_tensorf_checkpoint():
    from unboundednerfpytorch_amd.dcvgo_render import DirectContractedVoxGORenderer
    m = build('dcvgo', 11, width=128)
    ck = {'model_kwargs': m.get_kwargs(), 'model_state_dict': {k: v.detach().cpu().contiguous() for k, v in m.state_dict().items()}}
    rend = DirectContractedVoxGORenderer.from_tensorf_checkpoint(ck, DEV)
    assert rend.fused_supported() and torch.equal(rend.s['scene_radius'].cpu(), m.scene_radius.cpu())
    o, d, v = rays(256, 12, 'dcvgo')      # (inward-facing unbounded scene: cameras inside the separating cube)
    got = rend.render_rays(o, d, v, stepsize=0.5, bg=1)
    with torch.no_grad():
        want = m(o, d, v, stepsize=0.5, bg=1)
    assert float((want['alphainv_last'] < 0.99).float().mean()) > 0.2
    _same_as_model(got, want, o.shape[0])
