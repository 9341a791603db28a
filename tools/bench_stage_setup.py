"""Set-up time of the two training stages of the bounded model at config size (BASELINE configs[0], nerf_synthetic 'lego'), fused
against composed (train_rays.FUSED_SETUP on / off, alternating in one process):

  count    DirectVoxGO.voxel_count_views -- the coarse stage's per-voxel learning rate (run_train.py: pervoxel_lr) on the coarse model
           (num_voxels 1 024 000 over the lego box): per image two launches (ugrid_count_views_accumulate / _commit) against the
           autograd backward of a lookup on [10000, n_samples, 3] materialised points per chunk
  filter   dvgo_render.get_training_rays_in_maskcache_sampling -- the fine stage's ray table ('in_maskcache') on the fine model (160^3)
           with a coarse-geometry-like mask cache: per image one ugrid_hit_coarse_geo launch against sample_pts_on_rays (points + ids of
           every sample, a host read of their number), a boolean index, maskcache_lookup and a scatter

    python tools/bench_stage_setup.py [--views 20] [--hw 800] [--reps 2] [--out profiles/coarse/stage_setup.json]        (GPU box)

Synthetic views: cameras on a ring of radius 4.03 around the box, 30 degrees up, focal 1111 (the data set's).  One JSON document: per
(what, path) the wall time of every repetition in ms (host clock around work that ends in a device synchronise), its minimum, the
agreement of the two paths' results, and the board as the run found it (tools/board_state.py)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEGO_BOX = ([-0.67, -1.2, -0.37], [0.67, 1.2, 1.03])


def ring_views(n, hw):
    K = np.array([[1111.1 * hw / 800, 0, hw / 2], [0, 1111.1 * hw / 800, hw / 2], [0, 0, 1]], dtype=np.float32)
    centre = (np.array(LEGO_BOX[0]) + np.array(LEGO_BOX[1])) / 2
    poses = []
    for i in range(n):
        a, el = 2 * math.pi * i / n, math.radians(30)
        eye = centre + 4.03 * np.array([math.cos(a) * math.cos(el), math.sin(a) * math.cos(el), math.sin(el)])
        fwd = (centre - eye) / np.linalg.norm(centre - eye)
        right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        poses.append(np.stack([right, up, -fwd, eye], axis=1).astype(np.float32))      # OpenGL: x right, y up, looks along -z
    return K, poses


def model(num_voxels, coarse, dev):
    from unboundednerfpytorch_amd import voxgo_model as vm
    m = vm.DirectVoxGO(xyz_min=LEGO_BOX[0], xyz_max=LEGO_BOX[1], num_voxels=num_voxels, num_voxels_base=num_voxels,
                       alpha_init=1e-6 if coarse else 1e-2, fast_color_thres=1e-7 if coarse else 1e-4, rgbnet_dim=0 if coarse else 12,
                       rgbnet_direct=True).to(dev)
    if not coarse:
        # a coarse-geometry-like mask: an ellipsoid filling 60 % of the box's half extents (about a fifth of its volume)
        with torch.no_grad():
            xyz = m._vertices(m.mask_cache.mask.shape)
            c, h = (m.xyz_min + m.xyz_max) / 2, (m.xyz_max - m.xyz_min) / 2
            m.mask_cache.mask.copy_((((xyz - c) / (0.6 * h)) ** 2).sum(-1) <= 1)
    return m


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--hw", type=int, default=800)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse", "stage_setup.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_stage_setup.py measures on the GPU"
    import board_state
    from unboundednerfpytorch_amd import train_rays
    from unboundednerfpytorch_amd.dvgo_render import get_training_rays_in_maskcache_sampling
    from unboundednerfpytorch_amd.fourier_render import get_rays_of_a_view
    dev = torch.device("cuda", 0)
    H = W = args.hw
    K, poses = ring_views(args.views, args.hw)
    board = {"before": board_state.snapshot()}
    ro, rd = [], []
    for c2w in poses:
        o, d, _ = get_rays_of_a_view(H, W, torch.from_numpy(K).to(dev), torch.from_numpy(c2w).to(dev), inverse_y=False, flip_x=False, flip_y=False)
        ro.append(o.reshape(H, W, 3))
        rd.append(d.reshape(H, W, 3))
    o_tr, d_tr = torch.stack(ro), torch.stack(rd)
    del ro, rd
    coarse, fine = model(1024000, True, dev), model(160 ** 3, False, dev)
    imgs = [torch.rand(H, W, 3, device=dev) for _ in poses]
    rk = dict(near=2.0, far=6.0, stepsize=0.5)
    jobs = {
        "count": lambda: coarse.voxel_count_views(rays_o_tr=o_tr, rays_d_tr=d_tr, imsz=1, near=2.0, far=6.0, stepsize=0.5, downrate=1,
                                                  irregular_shape=False),
        "filter": lambda: get_training_rays_in_maskcache_sampling(imgs, [torch.from_numpy(p) for p in poses], [(H, W)] * len(poses),
                                                                  [K] * len(poses), False, False, False, False, fine, rk),
    }
    res = {"workload": "%d synthetic %d x %d views around the lego box; count: world_size %s, filter: world_size %s, mask %.3f occupied"
                       % (args.views, H, W, coarse.world_size.tolist(), fine.world_size.tolist(), float(fine.mask_cache.mask.float().mean())),
           "clock": "host perf_counter around the call, device synchronised before and after; paths alternate within a repetition",
           "reps": args.reps}
    try:
        for what, fn in jobs.items():
            ms = {"fused": [], "composed": []}
            last = {}
            for rep in range(args.reps):
                for path in ("fused", "composed"):
                    train_rays.FUSED_SETUP = path == "fused"
                    t, out = clocked(fn)
                    ms[path].append(round(t, 3))
                    last[path] = out
                    print(json.dumps({"what": what, "path": path, "rep": rep, "ms": round(t, 3)}), flush=True)
            res[what] = {p: {"ms": ms[p], "min_ms": min(ms[p])} for p in ms}
            res[what]["composed_over_fused"] = round(min(ms["composed"]) / min(ms["fused"]), 2)
            if what == "count":
                a, b = last["fused"], last["composed"]
                res[what]["voxels_that_differ"] = float((a != b).float().mean())
                res[what]["voxels_seen"] = int((a > 0).sum())
            else:
                a, b = last["fused"], last["composed"]
                res[what]["identical"] = bool(all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and list(a[4]) == list(b[4]))
                res[what]["rays_kept"] = int(a[0].shape[0])
                res[what]["rays"] = len(poses) * H * W
            del last
            torch.cuda.empty_cache()
    finally:
        train_rays.FUSED_SETUP = True
    board["after"] = board_state.snapshot()
    res["board"] = board
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
