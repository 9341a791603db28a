"""One iteration's ray batch at data-set size: `train_rays.sample_batch` on resident ray tables (four row gathers) against
`train_rays.sample_batch_lazy` on a RayBatcher (one ugrid_ray_batch launch, rays formed from the pose table), both arms alternating
in one process:

    python tools/bench_ray_batch.py [--views 250] [--h 1080] [--w 1920] [--iters 200] [--blocks 7] [--out profiles/ray_batch/batch.json]   (GPU box)

Synthetic views (seeded 8-bit images, cameras on a ring) of a non-FourierGrid model, so the table is 48 B a pixel (rgb, o, d,
viewdirs); for every (sampler in flatten / random) x (N_rand in 4096 / 8192) three arms: table, lazy on the float32 store, lazy on the
uint8 store.  A block is `iters` consecutive batches of one arm timed by the host clock between two device synchronisations; the
arms take turns block by block; reported per arm: the median block in microseconds per batch with the fastest and slowest block.
'flatten' draws from ONE epoch permutation per arm kind (host slices + a copy per batch for the table arm, one upload and device
slices for the lazy arms).  Resident bytes of each arm are differences of torch.cuda.memory_allocated around what the arm keeps.
The arms' batches are compared bit for bit under one seed before anything is timed."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def ring_poses(n):
    poses = []
    for i in range(n):
        a, el = 2 * math.pi * i / n, math.radians(20 + 10 * (i % 3))
        eye = 4.0 * np.array([math.cos(a) * math.cos(el), math.sin(a) * math.cos(el), math.sin(el)])
        fwd = -eye / np.linalg.norm(eye)
        right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
        up = np.cross(right, fwd)
        poses.append(np.stack([right, up, -fwd, eye], axis=1).astype(np.float32))
    return torch.from_numpy(np.stack(poses))


def block_us(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    del out
    return (time.perf_counter() - t0) * 1e6 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=250)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_batch", "batch.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ray_batch.py measures on the GPU"
    import board_state
    from unboundednerfpytorch_amd import train_rays as tr
    dev = torch.device("cuda", 0)
    N, H, W = args.views, args.h, args.w
    board = {"before": board_state.snapshot()}
    poses = ring_poses(N)
    K = np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]], dtype=np.float32)
    HW, Ks = np.array([(H, W)] * N), np.stack([K] * N)
    flags = dict(inverse_y=False, flip_x=False, flip_y=False)
    torch.manual_seed(0)
    alloc = lambda: torch.cuda.memory_allocated(dev)

    base = alloc()
    u8 = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev)
    lazy_u8 = tr.RayBatcher.from_views(u8, poses, HW, Ks, ndc=False, with_index=False, store="uint8", **flags)
    bytes_u8 = alloc() - base
    base = alloc()
    f32 = torch.empty((N, H, W, 3), dtype=torch.float32, device=dev)
    for i in range(N):
        f32[i] = (u8[i].double() / 255.).float()      # the loaders' (img / 255.).astype(np.float32)
    lazy_f32 = tr.RayBatcher.from_views(f32, poses, HW, Ks, ndc=False, with_index=False, store="float32", **flags)
    bytes_f32 = alloc() - base
    assert lazy_u8.images.data_ptr() == u8.data_ptr() and lazy_f32.images.data_ptr() == f32.data_ptr()
    base = alloc()
    table = tr.get_training_rays_flatten(f32, poses, HW, Ks, False, **flags)[:4]
    torch.cuda.synchronize()
    bytes_table = alloc() - base
    total = int(table[0].shape[0])
    res = {"workload": "%d synthetic %d x %d views (%d pixels), non-FourierGrid table: 48 B a pixel" % (N, W, H, total),
           "clock": "host perf_counter around %d consecutive batches, device synchronised before and after; the three arms take turns "
                    "block by block, %d blocks each; us per batch: median block [fastest, slowest]" % (args.iters, args.blocks),
           "resident_bytes": {"table": bytes_table, "lazy_float32": bytes_f32, "lazy_uint8": bytes_u8,
                              "table_over_lazy_float32": round(bytes_table / bytes_f32, 2), "table_over_lazy_uint8": round(bytes_table / bytes_u8, 2),
                              "note": "torch.cuda.memory_allocated differences; the table arm counts its own rgb rows (it does not need the "
                                      "images afterwards); by arithmetic 48 B (60 B with FourierGrid's index rows) against 12 B or 3 B a pixel "
                                      "plus 96 B a view"},
           "runs": []}
    for n_rand in (4096, 8192):
        t0 = time.perf_counter()
        np.random.seed(3)
        host_gen = tr.batch_indices_generator(total, n_rand)
        np.random.seed(3)
        dev_gen = tr.device_batch_indices_generator(total, n_rand, dev)
        for sampler in ("flatten", "random"):
            cfg = {"ray_sampler": sampler, "N_rand": n_rand}
            arms = {"table": lambda: tr.sample_batch(cfg, *table, None, lambda: next(host_gen)),
                    "lazy_float32": lambda: tr.sample_batch_lazy(cfg, lazy_f32, lambda: next(dev_gen)),
                    "lazy_uint8": lambda: tr.sample_batch_lazy(cfg, lazy_u8, lambda: next(dev_gen))}
            same = None
            if sampler == "random":                   # one seed, three arms: the same batch bit for bit
                outs = []
                for fn in arms.values():
                    torch.manual_seed(17)
                    outs.append(fn())
                same = all(torch.equal(a, b) for o in outs[1:] for a, b in zip(o[:4], outs[0][:4]))
            for fn in arms.values():                  # warm-up: code objects, the allocator's blocks, the epoch permutations
                block_us(fn, 20)
            setup_s = time.perf_counter() - t0
            us = {k: [] for k in arms}
            for _ in range(args.blocks):
                for k, fn in arms.items():
                    us[k].append(block_us(fn, args.iters))
            run = {"sampler": sampler, "N_rand": n_rand, "identical_batches": same,
                   "us_per_batch": {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                    for k, v in us.items()}}
            for k in ("lazy_float32", "lazy_uint8"):
                run["table_over_" + k] = round(statistics.median(us["table"]) / statistics.median(us[k]), 3)
            run["setup_s_before_timing"] = round(setup_s, 1)
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
    board["after"] = board_state.snapshot()
    res["board"] = board
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["resident_bytes"]), flush=True)


if __name__ == "__main__":
    main()
