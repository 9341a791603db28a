"""The training step of a TensoRF DirectVoxGO with the fused sampling march (TrainModel.fused_tensorf = True: grid.TrainSampleTensoRF,
and behind it ops.FusedRgbnet and ops.RenderLoss) against the composed, op-by-op forward (fused_tensorf = False), at
configs/nerf/ship.tensorf.py's final shape: world 384^3, density n_comp 8, k0 n_comp 24, rgbnet_dim 12, 3 x 128 rgbnet, 8192 rays,
stepsize 0.5, the fine stage's loss weights.

The scene is synthetic: one Gaussian blob of density (component 0 of the xy_plane / z_vec pair, a constant component for the empty
space, every other component N(0, 0.1) noise), its width searched until the composed path keeps --lo .. --hi stage-2 samples; the
occupancy cache is then the model's own (update_occupancy_cache).  The counts behind the mask cache, of stage 1 and of stage 2 are
recorded.  Rays: origins on a sphere of radius 3, each looking at a point near the blob, from a seed.

Timed: the model's forward as train_iteration calls it, and the whole train_iteration (forward, loss, backward, masked Adam; learning
rates 1e-12, so that the scene stays what was counted).  Arms: fused_tensorf False / True on ONE model in ONE process, alternating,
after a warm-up; each figure is the median of --blocks equal blocks of --iters calls, device events around a block.  Both factor
layouts.  The board's state is recorded before and after.

    python tools/bench_tensorf_train.py [--out profiles/tensorf/train_sample.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import board_state  # noqa: E402
from bench_tensorf import ab  # noqa: E402
from unboundednerfpytorch_amd import grid, ops, train_step as ts  # noqa: E402
from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model  # noqa: E402
from unboundednerfpytorch_amd.voxgo_model import DirectVoxGO  # noqa: E402

CFG = dict(lrate_density=1e-12, lrate_k0=1e-12, lrate_rgbnet=1e-12, lrate_decay=20, weight_main=1.0, weight_entropy_last=0.001,
           weight_rgbper=0.01, weight_nearclip=0.0, weight_distortion=0.0, tv_every=1, tv_after=0, tv_before=0, tv_dense_before=0,
           weight_tv_density=0.0, weight_tv_k0=0.0, skip_zero_grad_fields=['density', 'k0'])
RK = dict(near=0.2, far=6.0, stepsize=0.5, bg=1)
PEAK, FLOOR = 40.0, 6.0          # the blob's density at its centre is PEAK - FLOOR, the empty space's -FLOOR (alpha far below the threshold)


def build(world, comp_last, dev):
    torch.manual_seed(7)
    old = grid.TensoRFGrid.component_last
    grid.TensoRFGrid.component_last = comp_last
    try:
        m = DirectVoxGO(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=world ** 3, num_voxels_base=160 ** 3, alpha_init=1e-2,
                        fast_color_thres=1e-4, density_type='TensoRFGrid', density_config=dict(n_comp=8), k0_type='TensoRFGrid',
                        k0_config=dict(n_comp=24), rgbnet_dim=12, rgbnet_direct=True, rgbnet_width=128)
    finally:
        grid.TensoRFGrid.component_last = old
    return m.to(dev)


@torch.no_grad()
def set_blob(m, sigma):
    """density(x) = PEAK * exp(-|x|^2 / (2 sigma^2)) - FLOOR + what the other components' noise adds"""
    d = m.density
    X, Y, Z = [int(x) for x in m.world_size]
    g = lambda n: torch.exp(-torch.linspace(-1, 1, n, device=d.xy_plane.device) ** 2 / (2 * sigma * sigma))
    d.xy_plane[0, 0] = PEAK * g(X)[:, None] * g(Y)[None, :]
    d.z_vec[0, 0, :, 0] = g(Z)
    d.xy_plane[0, 1] = 1.0
    d.z_vec[0, 1, :, 0] = -FLOOR


def make_rays(n, dev, seed=11, aim=0.3):
    rs = np.random.RandomState(seed)
    o = rs.normal(size=(n, 3))
    o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rs.uniform(-aim, aim, (n, 3)) - o
    v = d / np.linalg.norm(d, axis=1, keepdims=True)
    return [torch.from_numpy(a.astype(np.float32)).to(dev) for a in (o, d, v)]


@torch.no_grad()
def counts(m, o, d):
    """the composed sampling, op by op: samples behind the mask cache, of stage 1 (alpha above the threshold), of stage 2 (weight too)"""
    pts, ray_id, _ = m.sample_ray(rays_o=o, rays_d=d, **RK)
    k = m.mask_cache(pts)
    pts, ray_id = pts[k], ray_id[k]
    alpha = m.activate_density(m.density(pts), RK['stepsize'] * m.voxel_size_ratio)
    k = alpha > m.fast_color_thres
    w, _ = ops.Alphas2Weights.apply(alpha[k], ray_id[k], o.shape[0])
    return {"mask_surviving": int(pts.shape[0]), "stage1": int(k.sum()), "stage2": int((w > m.fast_color_thres).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=384)
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--lo", type=int, default=100_000)
    ap.add_argument("--hi", type=int, default=200_000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"world": a.world, "rays": a.rays, "stepsize": RK['stepsize'], "density_n_comp": 8, "k0_n_comp": 24, "rgbnet_dim": 12,
           "board_before": board_state.snapshot(), "layouts": {}}
    o, d, v = make_rays(a.rays, dev)
    target = (0.5 + 0.4 * torch.sin(3.0 * v + torch.tensor([0.0, 1.0, 2.0], device=dev))).contiguous()
    sigma, search = None, []
    for layout in ("canonical", "complast"):
        m = build(a.world, layout == "complast", dev)
        if sigma is None:
            # the blob's width, by bisection on its logarithm, until the stage-2 count is inside [lo, hi] (it grows with the width)
            lo_s, hi_s = 0.01, 0.6
            for _ in range(16):
                sigma = math.sqrt(lo_s * hi_s)
                set_blob(m, sigma)
                c = counts(m, o, d)
                search.append({"sigma": sigma, **c})
                if a.lo <= c["stage2"] <= a.hi:
                    break
                lo_s, hi_s = (sigma, hi_s) if c["stage2"] < a.lo else (lo_s, sigma)
            else:
                raise SystemExit("no blob width gives %d .. %d stage-2 samples: %s" % (a.lo, a.hi, search))
        set_blob(m, sigma)
        m.update_occupancy_cache()
        case = {"world_size": [int(x) for x in m.world_size], "sigma": sigma, "counts": counts(m, o, d),
                "mask_cache_true_fraction": float(m.mask_cache.mask.float().mean())}
        opt = create_optimizer_or_freeze_model(m, CFG, global_step=0)
        coef = ops.loss_coefficients(CFG, a.rays, m.sample_table(RK['stepsize'], dev).numel(), None, 1)
        fkw = dict(RK, fused_loss={'target': target, 'coef': coef})
        step = [0]

        def forward(fused):
            m.fused_tensorf = fused
            return m(o, d, v, global_step=1, is_train=True, **fkw)

        def iteration(fused):
            m.fused_tensorf = fused
            step[0] += 1
            return ts.train_iteration(m, opt, o, d, v, target, CFG, step[0], RK, return_tensors=True)
        fa, fb = forward(True), forward(False)
        case["same_samples"] = bool(torch.equal(fa['ray_id'], fb['ray_id']) and torch.equal(fa['weights'], fb['weights']))
        case["stage2_fused"] = int(fa['ray_id'].numel())
        case["fused_tail"] = 'loss' in fa and 'loss' not in fb          # (ops.RenderLoss comes with the fused sampling)
        del fa, fb
        case["forward"] = ab({"composed": lambda: forward(False), "fused": lambda: forward(True)}, a.iters, a.blocks)
        case["train_iteration"] = ab({"composed": lambda: iteration(False), "fused": lambda: iteration(True)}, a.iters, a.blocks)
        case["counts_after"] = counts(m, o, d)
        res["layouts"][layout] = case
        del m, opt
        torch.cuda.empty_cache()
    res["blob_search"] = search
    res["board_after"] = board_state.snapshot()
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    for layout, case in res["layouts"].items():
        print(layout, case["counts"], "same samples:", case["same_samples"])
        for what in ("forward", "train_iteration"):
            r = case[what]
            print("  %s: composed %.3f ms, fused %.3f ms" % (what, r["composed"]["median_ms"], r["fused"]["median_ms"]))


if __name__ == "__main__":
    main()
