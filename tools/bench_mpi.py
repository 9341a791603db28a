"""Forward-facing DirectMPIGO render on one MI355X: a 1008 x 756 LLFF view (configs/llff) of a trained-like scene through the
fused march (ugrid_render_march_mpi) + shade kernels, against the composed forward over the drop-in ops chunked at 8192
rays as the reference's render loop chunks it (run_render.py:52-58).  Two shapes:
  S_default  256^3 voxels, mpi_depth 128, stepsize 0.5   (llff_default.py)
  S_lg       384^2 x 256, mpi_depth 256, stepsize 1.0    (llff_default_lg.py)
Prints one JSON line per shape: median fused march / shade times (events around each launch), fused frame time, composed
frame time, samples marched.

    python tools/bench_mpi.py [--reps 10] [--composed-reps 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(D, nvox, stepsize, seed=7):
    """trained-like grids: a few smooth surfaces (density bumps along z per pixel column) plus noise, free space masked"""
    from unboundednerfpytorch_amd.mpi_render import mpi_state_from_params
    lo, hi = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
    t = torch.Tensor(lo), torch.Tensor(hi)
    r = (nvox / D / (t[1] - t[0])[:2].prod()).sqrt()
    X, Y = [int(x) for x in ((t[1] - t[0])[:2] * r)]
    g = torch.Generator().manual_seed(seed)
    xs, ys = torch.linspace(-1, 1, X), torch.linspace(-1, 1, Y)
    surf = 0.3 + 0.25 * torch.sin(3 * xs)[:, None] * torch.cos(2 * ys)[None, :]           # depth of the front surface, [X,Y] in (0,1)
    z = torch.linspace(0, 1, D)
    dens = 30.0 * torch.exp(-((z[None, None, :] - surf[..., None]) / 0.02) ** 2) - 8.0
    dens += 0.5 * torch.randn(X, Y, D, generator=g)
    k0 = 0.5 * torch.randn(1, 9, X, Y, D, generator=g)
    mask = dens > -6.0
    w = [torch.randn(64, 12, generator=g) * 0.3, torch.randn(64, 64, generator=g) * 0.12, torch.randn(3, 64, generator=g) * 0.12]
    b = [torch.zeros(64), torch.zeros(64), torch.zeros(3)]
    shift = torch.zeros(1, 1, 1, 1, D)
    return mpi_state_from_params(lo, hi, nvox, D, dens[None, None], shift, k0, w, b, mask, stepsize / D / 5, 0)


def bench(name, D, nvox, stepsize, reps, composed_reps):
    from unboundednerfpytorch_amd.fourier_render import get_rays_of_a_view, get_rays_of_pixel_index, pixel_tile_order
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    H, W = 756, 1008
    K = np.array([[820.0, 0, W / 2], [0, 820.0, H / 2], [0, 0, 1]])
    c2w = torch.tensor([[1.0, 0, 0, 0.02], [0, 1.0, 0, -0.01], [0, 0, 1.0, 0.0]], device="cuda")
    rend = DirectMPIGORenderer(scene(D, nvox, stepsize), "cuda:0")
    assert rend.fused_supported()
    kw = dict(near=0, far=1, stepsize=stepsize, bg=1, render_depth=True)
    order = pixel_tile_order(H, W, "cuda:0")      # (None at 756 rows: not a multiple of 8 -- render_view renders in image order)
    if order is not None:
        o, d, v = get_rays_of_pixel_index(H, W, K, c2w, order, ndc=True)
    else:
        o, d, v = [x.reshape(-1, 3).contiguous() for x in get_rays_of_a_view(H, W, K, c2w, ndc=True)]
    for _ in range(2):
        rend.render_view(H, W, K, c2w, **kw)
    torch.cuda.synchronize()
    frame, march, shade = [], [], []
    for _ in range(reps):
        timing = []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rend.render_view(H, W, K, c2w, timing=timing, **kw)
        e1.record()
        torch.cuda.synchronize()
        frame.append(e0.elapsed_time(e1))
        march.append(sum(ev[0].elapsed_time(ev[1]) for ev, _ in timing))
        shade.append(sum(ev[1].elapsed_time(ev[2]) for ev, _ in timing))
    fused = rend._fused_renderer()
    fused(o, d, v, ray_order="coherent", **kw)
    surv = fused.survivors_of_last_chunk()
    comp = []
    for _ in range(composed_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for bs in range(0, H * W, 8192):
            rend(o[bs:bs + 8192], d[bs:bs + 8192], v[bs:bs + 8192], **kw)
        torch.cuda.synchronize()
        comp.append((time.perf_counter() - t0) * 1e3)
    n = rend.n_samples(stepsize)
    res = {"shape": name, "H": H, "W": W, "world_size": rend.s["world_size"].tolist(), "mpi_depth": D, "stepsize": stepsize,
           "samples_per_ray": n, "samples": H * W * n, "survivors": surv,
           "fused_march_ms": float(np.median(march)), "fused_shade_ms": float(np.median(shade)),
           "fused_frame_ms": float(np.median(frame)), "composed_frame_ms": float(np.median(comp)),
           "speedup": float(np.median(comp) / np.median(frame)), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--composed-reps", type=int, default=2)
    a = ap.parse_args()
    bench("S_default", 128, 256 ** 3, 0.5, a.reps, a.composed_reps)
    bench("S_lg", 256, 384 * 384 * 256, 1.0, a.reps, a.composed_reps)


if __name__ == "__main__":
    main()
