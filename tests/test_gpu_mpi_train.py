"""mpi_model.DirectMPIGO on the GPU -- the fused training forward of forward-facing (NDC) scenes (k_train_march_vox<3> through
grid.TrainSampleVox('mpi'), ugrid_train_sample_mpi) -- against the fixtures the reference's OWN dmpigo.DirectMPIGO wrote on the CPU
(tests/golden/gen_mpi_train_golden.py: one training forward + backward of both MPI_CASES, update_occupancy_cache, scale_volume_grid)
and against the op-by-op chain over the drop-in ops on the same device.

The shapes are tests/mpi_cases.py's (mpi_depth 24 / 16, ~10 k voxels, 300 / 200 rays): n_steps 47 and 16 -- a partial wave of the
64-sample rounds --, rays that leave the box in x / y, samples on the last plane of the shift table; n_steps 511 (mpi_depth 256)
in the edge-case test walks eight rounds."""
import os
import sys

import numpy as np
import pytest
import torch

import mpi_cases
import synth
from test_mpi_train import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
IDS = [c[0] for c in mpi_cases.MPI_CASES]
pytestmark = pytest.mark.gpu


def golden_loss(out, target, R):
    """test_gpu_voxgo_train.golden_loss' terms (DirectMPIGO returns no raw density)"""
    loss = torch.nn.functional.mse_loss(out["rgb_marched"], target)
    p = out["alphainv_last"].clamp(1e-6, 1 - 1e-6)
    loss = loss + 0.01 * (-(p * torch.log(p) + (1 - p) * torch.log(1 - p))).mean()
    return loss + 0.05 * (out["weights"] * out["weights"]).sum() / R


def sample_keys(ray_id, s, n):
    """(ray_id, step) of every sample as one integer: step = round(s * N - 0.5)"""
    step = np.rint(np.asarray(s, dtype=np.float64) * n - 0.5).astype(np.int64)
    assert step.min(initial=0) >= 0 and step.max(initial=0) < n
    return np.asarray(ray_id, dtype=np.int64) * n + step


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=IDS)
def test_fused_training_forward_backward_matches_the_reference_model(case):
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    dev = torch.device("cuda", 0)
    m, (o, d, v), kw = build(case, dev)
    gold = np.load(os.path.join(GOLD, "mpi_train_" + name + ".npz"))
    target = torch.from_numpy(gold["target"]).to(dev)
    assert m.fused_forward and m._can_fuse(o)
    out = m(o, d, v, global_step=1, **kw)
    if C > 0:       # llff's Linear(12,64)-ReLU-Linear(64,64)-ReLU-Linear(64,3) without view frequencies runs on ops.FusedRgbnet
        from unboundednerfpytorch_amd import ops
        assert m.fused_rgbnet and ops.rgbnet_linears(m.rgbnet) is not None and m.viewfreq.numel() == 0
        node, seen = out["raw_rgb"].grad_fn, set()
        while node is not None and "FusedRgbnet" not in type(node).__name__:
            seen.add(type(node).__name__)
            node = node.next_functions[0][0] if node.next_functions else None
        assert node is not None, sorted(seen)
    loss = golden_loss(out, target, R)
    loss.backward()
    torch.cuda.synchronize()
    n = int(gold["n_max"])
    assert out["n_max"] == n and out["s"].dtype == torch.float32
    assert int(gold["n_kept"]) >= 500
    got = {k: out[k].detach().cpu().numpy() for k in ("weights", "raw_alpha", "raw_rgb", "ray_id", "s", "rgb_marched", "alphainv_last",
                                                      "depth")}
    kg, kr = sample_keys(got["ray_id"], got["s"], n), sample_keys(gold["ray_id"], gold["s"], n)
    assert np.all(np.diff(kg) > 0) and np.all(np.diff(kr) > 0)            # ray-major, near to far, no sample twice
    # a ray whose sample set differs from the reference's (a 1-ulp alpha or weight at a threshold) is left out of the per-sample and
    # per-ray comparisons: at most 2 per case
    odd = np.union1d(np.setdiff1d(kg, kr) // n, np.setdiff1d(kr, kg) // n)
    print("%s: kept %d (reference %d), rays left out %s" % (name, kg.size, kr.size, odd.tolist()))
    assert odd.size <= 2, odd
    sg, sr = ~np.isin(got["ray_id"], odd), ~np.isin(gold["ray_id"], odd)
    assert np.array_equal(kg[sg], kr[sr])
    # s = (step + 0.5) / N: torch divides by a Python number with an IEEE division on the CPU (the fixture) and with a multiplication
    # by the rounded reciprocal on the device -- 1.5 ulp of a value below 1 apart at the most (3 * 2^-25 < 1e-7)
    np.testing.assert_allclose(got["s"][sg], gold["s"][sr], rtol=0, atol=1e-7)
    for k in ("weights", "raw_alpha", "raw_rgb"):
        err = float(np.abs(got[k][sg] - gold[k][sr]).max())
        print("  %s max err %.3g" % (k, err))
        assert err <= 2e-5, (k, err)
    rays = ~np.isin(np.arange(R), odd)
    for k in ("rgb_marched", "alphainv_last", "depth"):
        err = float(np.abs(got[k][rays] - gold[k][rays]).max())
        print("  %s max err %.3g" % (k, err))
        assert err <= 1e-4, (k, err)
    print("  loss %.8f reference %.8f" % (float(loss), float(gold["loss"])))
    np.testing.assert_allclose(float(loss), float(gold["loss"]), rtol=2e-5)
    assert m.act_shift.grid.grad is None
    names = [k for k, p in m.named_parameters() if p.requires_grad]
    assert sorted("grad." + k for k in names) == sorted(k for k in gold.files if k.startswith("grad."))
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        g = gold["grad." + k]
        assert p.grad is not None, k
        scale = float(np.abs(g).max()) + 1e-20
        err = float(np.abs(p.grad.cpu().numpy() - g).max())
        print("  grad %s err / max %.3g" % (k, err / scale))
        assert err <= 5e-4 * scale, (k, err / scale)
        if "grid" in k and odd.size == 0:
            assert np.array_equal(p.grad.cpu().numpy() != 0, g != 0), k          # the voxels MaskedAdam will update


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=IDS)
def test_fused_sampling_equals_the_op_by_op_chain(case):
    """fused (one march + one compaction) vs composed (sample_ndc_pts_on_rays / maskcache_lookup / two grid queries / Raw2Alpha /
    Alphas2Weights as separate drop-in ops) on the same device, some rays moved outside the box: the same samples, values within
    the bars test_gpu_voxgo_train.py applies to DirectContractedVoxGO"""
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    dev = torch.device("cuda", 0)
    m, (o, d, v), kw = build(case, dev)
    target = torch.from_numpy(synth.uniform(seed + 5, R * 3).reshape(R, 3).astype(np.float32)).to(dev)
    o = o.clone()
    o[:5, :2] = o[:5, :2] * 6.0            # outside the box in x / y: some never enter, some cross it
    o[5, 2] = -3.0                         # starts before the near plane
    res = {}
    for fused in (True, False):
        m.fused_forward = fused
        m.zero_grad(set_to_none=True)
        out = m(o, d, v, global_step=1, **kw)
        golden_loss(out, target, R).backward()
        res[fused] = (out, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    a, b = res[True][0], res[False][0]
    assert a["weights"].numel() > 500
    for k in ("ray_id", "s"):
        assert torch.equal(a[k], b[k]), k
    differ = []
    for k in ("weights", "raw_alpha", "alphainv_last", "raw_rgb"):
        err = float((a[k] - b[k]).abs().max())
        differ += [] if torch.equal(a[k], b[k]) else [(k, err)]
        assert err <= 2e-6, (k, err)
    for k in ("rgb_marched", "depth"):
        err = float((a[k] - b[k]).abs().max())
        differ += [] if torch.equal(a[k], b[k]) else [(k, err)]
        assert err <= 5e-6, (k, err)
    print("%s: fused vs op-by-op outputs not bit-equal: %s" % (name, differ or "none"))
    assert sorted(res[True][1]) == sorted(res[False][1])
    for k in res[True][1]:
        ga, gb = res[True][1][k], res[False][1][k]
        scale = float(gb.abs().max()) + 1e-20
        print("  grad %s diff / max %.3g, same nonzero pattern %s" % (k, float((ga - gb).abs().max()) / scale, torch.equal(ga != 0, gb != 0)))
        assert float((ga - gb).abs().max()) <= 1e-4 * scale, (k, float((ga - gb).abs().max()) / scale)


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=IDS)
def test_occupancy_cache_and_coarse_to_fine_step_match_the_reference(case):
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    dev = torch.device("cuda", 0)
    m, (o, d, v), kw = build(case, dev)
    gold = np.load(os.path.join(GOLD, "mpi_train_" + name + ".npz"))
    m.update_occupancy_cache()
    got = m.mask_cache.mask.cpu().numpy()
    assert 0 < int(gold["occ_mask"].sum()) < gold["occ_mask"].size
    assert int((got != gold["occ_mask"]).sum()) <= 2            # (alpha > thres at a vertex: a 1-ulp flip at most)
    m.scale_volume_grid(2 * nvox, D)
    assert m.world_size.tolist() == gold["scaled_world_size"].tolist() and m.mpi_depth == D and m.voxel_size_ratio == 256. / D
    np.testing.assert_allclose(m.density.grid.detach().cpu().numpy(), gold["scaled_density"], rtol=0, atol=2e-5)
    ch = gold["scaled_k0_channels"].tolist()
    k0s = m.k0.grid.detach().cpu().numpy()
    np.testing.assert_allclose(k0s[:, ch], gold["scaled_k0"], rtol=0, atol=2e-5)
    rest = gold["scaled_k0_rest_channels"].tolist()          # stored rounded to fp16 (2^-11 relative): the same bar + that rounding
    assert sorted(ch + rest) == list(range(k0s.shape[1]))
    if rest:
        want = gold["scaled_k0_rest_f16"].astype(np.float32)
        assert bool((np.abs(k0s[:, rest] - want) <= 2e-5 + 2.0 ** -11 * np.abs(want)).all())
    assert list(m.k0.grid.shape) == [1, max(C, 3)] + gold["scaled_world_size"].tolist()
    assert float((m.mask_cache.mask.cpu().numpy() != gold["scaled_mask"]).mean()) <= 2e-3
    with torch.no_grad():
        out = m(o, d, v, global_step=2, **kw)       # the fused forward on the rescaled model (new mask, new world size)
    assert abs(int(out["weights"].numel()) - int(gold["scaled_n_kept"])) <= max(4, int(0.004 * int(gold["scaled_n_kept"])))
    np.testing.assert_allclose(out["rgb_marched"].cpu().numpy(), gold["scaled_rgb_marched"], rtol=0, atol=2e-3)


LOOP_STEPS, LOOP_SCALE_AT = 30, 10


def run_training_loop(fused, steps=LOOP_STEPS):
    """train_step.train_iteration on the fine case for `steps` steps across one pg_scale event, llff_default's loss weights
    (configs/llff/llff_default.py + default.py's fine_train): distortion 0.01, entropy_last 0.001, rgbper 0.01, TV 1e-5 / 1e-6 dense,
    then masked, decay_after_scale 1.0.  -> (losses, psnrs, model)"""
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model
    case = mpi_cases.MPI_CASES[0]
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    dev = torch.device("cuda", 0)
    m, (o, d, v), kw = build(case, dev)
    m.fused_forward = fused
    with torch.no_grad():
        m.mask_cache.mask.fill_(True)
    target = torch.from_numpy(synth.uniform(seed + 5, R * 3).reshape(R, 3).astype(np.float32)).to(dev) * 0.5 + 0.25
    cfg_train = dict(lrate_density=1e-1, lrate_k0=1e-1, lrate_rgbnet=1e-3, lrate_decay=20, pg_scale=[LOOP_SCALE_AT], decay_after_scale=1.0,
                     weight_main=1.0, weight_entropy_last=0.001, weight_rgbper=0.01, weight_nearclip=0.0, weight_distortion=0.01,
                     tv_every=1, tv_after=0, tv_before=1e9, tv_dense_before=LOOP_SCALE_AT + 6, weight_tv_density=1e-5, weight_tv_k0=1e-6,
                     skip_zero_grad_fields=['density', 'k0'])
    cfg_model = dict(num_voxels=nvox * 2)
    opt = create_optimizer_or_freeze_model(m, cfg_train, global_step=0)
    rk = {k: kw[k] for k in kw if k != "render_depth"}
    shift0 = m.act_shift.grid.detach().clone()
    losses, psnrs = [], []
    for step in range(1, steps + 1):
        opt = ts.maybe_scale_grids(m, opt, cfg_train, cfg_model, step)
        loss, psnr = ts.train_iteration(m, opt, o, d, v, target, cfg_train, step, rk)
        losses.append(loss)
        psnrs.append(psnr)
    torch.cuda.synchronize()
    assert int(m.num_voxels) == nvox * 2 and m.world_size.tolist() == mpi_cases.world_size(nvox * 2, D)
    assert torch.equal(m.act_shift.grid, shift0 - 1.0)          # decay_after_scale reached the per-plane shift, nothing else did
    return losses, psnrs, m


# final PSNR of the OP-BY-OP loop below, four runs on one MI355X: 14.043274, 14.043274, 14.043280, 14.043279 dB -- max - min = 6e-6 dB
# (its scatters add with float atomics in an order that differs from run to run; 30 Adam steps carry that into the last digits of
# a float32 PSNR, whose spacing at 14 dB is 1e-6).  The fused loop may end 2 x that spread from an op-by-op run.
LOOP_SPREAD_DB = 6e-6


def test_training_loop_learns_and_ends_where_the_op_by_op_loop_does():
    """30 steps of train_iteration across a pg_scale event: the loss is finite and goes down, and the fused loop ends where the
    op-by-op loop (fused_forward = False) ends, to 2 x the op-by-op loop's own run-to-run spread (LOOP_SPREAD_DB)."""
    losses, psnrs, m = run_training_loop(True)
    print("fused loop: losses", ["%.5f" % x for x in losses])
    assert all(np.isfinite(losses)) and all(np.isfinite(psnrs))
    for p in m.parameters():
        assert bool(torch.isfinite(p).all())
    # decreasing on the fixed batch within each resolution (the scale step lowers the density bias by 1: the loss jumps there)
    assert losses[LOOP_SCALE_AT - 2] < losses[0] and losses[-1] < losses[LOOP_SCALE_AT - 1], losses
    ref = run_training_loop(False)[1][-1]
    print("final psnr: fused %.6f, op-by-op %.6f, difference %.2g dB (allowed %.2g)" % (psnrs[-1], ref, abs(psnrs[-1] - ref), 2 * LOOP_SPREAD_DB))
    assert abs(psnrs[-1] - ref) <= 2 * LOOP_SPREAD_DB, (psnrs[-1], ref)


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=IDS)
def test_two_fused_forwards_are_bit_identical(case):
    """what the march, the compaction, the k0 lookup and the rgbnet produce carries no atomics: bit-identical between two calls, and
    so is the fused tail (ops.RenderLoss: per-ray sums in sample order).  The composed tail's rgb_marched / depth are index_add_
    sums (float atomics, the order differs between runs): equal to the reordering error of a ray's <= N_samples terms, each
    at most 1 -- N * 2^-24 * (the ray's sum <= 1) < 5e-6 for N = 47."""
    from unboundednerfpytorch_amd.ops import loss_coefficients
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    dev = torch.device("cuda", 0)
    m, (o, d, v), kw = build(case, dev)
    with torch.no_grad():
        a = m(o, d, v, global_step=1, **kw)
        b = m(o, d, v, global_step=1, **kw)
    assert a["weights"].numel() > 500
    for k in ("alphainv_last", "weights", "raw_alpha", "raw_rgb", "ray_id", "s"):
        assert torch.equal(a[k], b[k]), k
    for k in ("rgb_marched", "depth"):
        assert float((a[k] - b[k]).abs().max()) <= 5e-6, k
    target = torch.from_numpy(synth.uniform(seed + 5, R * 3).reshape(R, 3).astype(np.float32)).to(dev)
    cfg = dict(weight_main=1.0, weight_entropy_last=0.01, weight_rgbper=0.02, weight_distortion=0.05, weight_nearclip=0.0)
    fl = {'target': target, 'coef': loss_coefficients(cfg, R, m.sample_table(stepsize, dev).numel(), None, 1)}
    rk = {k: kw[k] for k in kw if k != "render_depth"}
    with torch.no_grad():
        a = m(o, d, v, global_step=1, fused_loss=fl, **rk)
        b = m(o, d, v, global_step=1, fused_loss=fl, **rk)
    for k in ("loss", "mse", "rgb_marched", "raw_logits", "weights", "alphainv_last"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=IDS)
def test_fused_loss_equals_the_composed_loss(case):
    """the training tail as one op (ops.RenderLoss with s = (step + 0.5) / N passed explicitly, what train_iteration selects) vs the
    torch chain of train_step.training_loss on the model's return dict: the same loss and gradients -- entropy, rgbper, distortion,
    the bg = 1 background; fine (rgbnet) and coarse (k0 = colour) stage.  Bars: test_gpu_voxgo_train.test_fused_loss_equals_the_composed_loss'"""
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.ops import loss_coefficients
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    dev = torch.device("cuda", 0)
    m, (o, d, v), kw = build(case, dev)
    target = torch.from_numpy(synth.uniform(seed + 5, R * 3).reshape(R, 3).astype(np.float32)).to(dev)
    cfg = dict(weight_main=1.0, weight_entropy_last=0.01, weight_rgbper=0.02, weight_distortion=0.05, weight_nearclip=0.0)
    rk = {k: kw[k] for k in kw if k != "render_depth"}
    res = {}
    for fused in (True, False):
        m.zero_grad(set_to_none=True)
        if fused:
            coef = loss_coefficients(cfg, R, m.sample_table(stepsize, dev).numel(), None, 1)
            out = m(o, d, v, global_step=1, is_train=True, fused_loss={'target': target, 'coef': coef}, **rk)
            assert "loss" in out and out["n_max"] == m.n_samples(stepsize)
            loss = out["loss"]
        else:
            out = m(o, d, v, global_step=1, is_train=True, **rk)
            loss, _ = ts.training_loss(out, target, cfg, R)
        loss.backward()
        res[fused] = (float(loss), out["rgb_marched"].detach(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    print("%s: fused loss %.8f composed %.8f" % (name, res[True][0], res[False][0]))
    assert abs(res[True][0] - res[False][0]) <= 2e-6 * abs(res[False][0]), (res[True][0], res[False][0])
    assert float((res[True][1] - res[False][1]).abs().max()) <= 2e-6
    assert sorted(res[True][2]) == sorted(res[False][2])
    for k in res[True][2]:
        ga, gb = res[True][2][k], res[False][2][k]
        scale = float(gb.abs().max()) + 1e-20
        assert float((ga - gb).abs().max()) <= 2e-4 * scale, (k, float((ga - gb).abs().max()) / scale)


def test_occupancy_lt_nviews_keeps_what_the_views_see():
    """DirectMPIGO.update_occupancy_cache_lt_nviews (dmpigo.py:189-207), as test_gpu_voxgo_train checks DCVGO's: the mask only loses
    voxels, some are seen and some never, and nothing is kept that no sample comes near"""
    dev = torch.device("cuda", 0)
    name, seed, D, nvox, C, stepsize, R, dm, ds = mpi_cases.MPI_CASES[0]
    m, (o, d, v), kw = build(mpi_cases.MPI_CASES[0], dev)
    with torch.no_grad():
        m.mask_cache.mask.fill_(True)
    o, d = o * torch.tensor([0.5, 0.5, 1.0], device=dev), d * torch.tensor([0.5, 0.5, 1.0], device=dev)      # a narrower bundle
    rk = dict(near=0, far=1, stepsize=stepsize)
    m.update_occupancy_cache_lt_nviews(o, d, [R // 3] * 3, rk, maskout_lt_nviews=1)
    mask = m.mask_cache.mask
    frac = float(mask.float().mean())
    assert 0.02 < frac < 0.98, frac
    pts = m.sample_ray(rays_o=o, rays_d=d, **rk)[0]
    shape = torch.tensor(list(mask.shape), device=dev)
    idx = ((pts - m.xyz_min) / (m.xyz_max - m.xyz_min) * (shape - 1)).round().long()
    idx = torch.minimum(torch.maximum(idx, torch.zeros_like(idx)), shape - 1)
    touched = torch.zeros_like(mask)
    touched[idx[:, 0], idx[:, 1], idx[:, 2]] = True
    near_any = torch.nn.functional.max_pool3d(touched[None, None].float(), 3, 1, 1)[0, 0] > 0
    assert not bool((mask & ~near_any).any())


def test_edge_cases_few_rays_a_miss_and_the_deepest_table():
    dev = torch.device("cuda", 0)
    case = mpi_cases.MPI_CASES[0]
    m, (o, d, v), kw = build(case, dev)
    # R = 5 (less than one block of four waves + a ragged tail), ray 2 misses the box entirely
    o5, d5, v5 = o[:5].clone(), d[:5].clone(), v[:5].clone()
    o5[2] = torch.tensor([5.0, 5.0, -1.0], device=dev)
    d5[2] = torch.tensor([0.0, 0.0, 2.0], device=dev)
    res = {}
    for fused in (True, False):
        m.fused_forward = fused
        with torch.no_grad():
            res[fused] = m(o5, d5, v5, global_step=1, **kw)
    a, b = res[True], res[False]
    assert a["rgb_marched"].shape == (5, 3) and a["weights"].numel() > 0
    assert int((a["ray_id"] == 2).sum()) == 0 and float(a["alphainv_last"][2]) == 1.0
    assert torch.equal(a["rgb_marched"][2], torch.ones(3, device=dev)) and float(a["depth"][2]) == 0.0      # bg = 1
    assert torch.equal(a["ray_id"], b["ray_id"]) and torch.equal(a["s"], b["s"])
    for k in ("weights", "alphainv_last", "rgb_marched"):
        assert float((a[k] - b[k]).abs().max()) <= 5e-6, k
    # every ray misses: empty sample lists, every count 0
    m.fused_forward = True
    with torch.no_grad():
        e = m(o5[2:3].expand(3, 3).contiguous(), d5[2:3].expand(3, 3).contiguous(), v5[:3], global_step=1, **kw)
    assert e["weights"].numel() == 0 and torch.equal(e["alphainv_last"], torch.ones(3, device=dev))
    # mpi_depth = 256: the largest shift table the kernel takes, n_steps = 511 (eight rounds of 64 samples), z planes 0 .. 255
    from unboundednerfpytorch_amd.mpi_model import DirectMPIGO
    torch.manual_seed(7)
    big = DirectMPIGO(xyz_min=mpi_cases.XYZ_MIN, xyz_max=mpi_cases.XYZ_MAX, num_voxels=256 * 6 * 5, mpi_depth=256,
                      fast_color_thres=mpi_cases.fast_color_thres(0.5, 256), rgbnet_dim=0)
    assert big.world_size.tolist()[2] == 256 and big.n_samples(0.5) == 511
    with torch.no_grad():
        big.density.grid.copy_(torch.randn(big.density.grid.shape) * 1.5 - 1.5)
        big.k0.grid.copy_(torch.randn(big.k0.grid.shape))
    big = big.to(dev)
    kb = dict(near=0, far=1, stepsize=0.5, bg=1, render_depth=True)
    res = {}
    for fused in (True, False):
        big.fused_forward = fused
        with torch.no_grad():
            res[fused] = big(o[:40], d[:40], v[:40], global_step=1, **kb)
    a, b = res[True], res[False]
    assert a["n_max"] == 511 and a["weights"].numel() > 500
    assert torch.equal(a["ray_id"], b["ray_id"]) and torch.equal(a["s"], b["s"])
    assert float(a["s"].max()) > 0.9                      # samples up to the far planes survive (the initial shift equalises alpha)
    for k in ("weights", "raw_alpha", "alphainv_last"):
        assert float((a[k] - b[k]).abs().max()) <= 2e-6, k
    for k in ("rgb_marched", "depth"):
        assert float((a[k] - b[k]).abs().max()) <= 5e-6, k
    # a table deeper than 256 planes is refused, not mis-read
    from unboundednerfpytorch_amd import grid as G
    cfg = {'mode': 'mpi', 'interval': 1.0, 'thres': 1e-3, 'mask_scale': [1.0] * 3, 'mask_shift': [0.0] * 3, 'n_steps': 4,
           'mpi_depth': 257, 'act_shift': torch.zeros(257, device=dev)}
    with pytest.raises(RuntimeError):
        G.TrainSampleVox.apply(big.density.grid, o[:4].contiguous(), d[:4].contiguous(), None, big.xyz_min, big.xyz_max,
                               big.mask_cache.mask, cfg)
