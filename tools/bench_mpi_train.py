"""Training-step time of the forward-facing model at llff_default's fine-stage size (configs/llff/llff_default.py: num_voxels
256^3, mpi_depth 128, rgbnet_dim 9, width 64, N_rand 4096, stepsize 0.5, distortion 1e-2, entropy_last 1e-3, rgbper 1e-2, TV density
1e-5 / k0 1e-6, dense before step 10 000) through mpi_model.DirectMPIGO + train_step.train_iteration (the loop body of
run_train.py:185-296): the FUSED step (grid.TrainSampleVox 'mpi' + ops.RenderLoss) against the OP-BY-OP step of the same model
(fused_forward = False: sample_ndc_pts_on_rays, maskcache_lookup, two grid queries, Raw2Alpha, Alphas2Weights, the boolean-index
compactions between them, the composed compositing and loss), ALTERNATING step by step on the same model and optimizer, every
step clocked on the host between device synchronisations; the medians are reported.

    python tools/bench_mpi_train.py [--steps 20] [--warmup 4] [--phase dense|masked|both] [--out profiles/mpi/bench_mpi_train.txt]

`--arms native` measures what the native step (native_step.VoxGOStep mode 'mpi') is worth instead, three arms alternating in the same
way: (a) the fused op-by-op step (native_step = False: four autograd nodes, the yardstick), (b) the native step with its one host
read, (c) the native step sync-free (native_sync_free = True, train_iteration(return_tensors=True): no host read in the step; the
clock still stops at a device synchronisation).  Default --out then: profiles/mpi/bench_mpi_train_native.txt.

One JSON line per TV phase.  Trained-like grids (tools/bench_mpi.py's scene: a smooth front surface + noise, free space masked),
4096 random rays of a 1008 x 756 NDC view per step."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CFG = dict(N_rand=4096, weight_main=1.0, weight_entropy_last=1e-3, weight_rgbper=1e-2, weight_nearclip=0.0, weight_distortion=1e-2,
           weight_tv_density=1e-5, weight_tv_k0=1e-6, tv_before=1e9, tv_dense_before=10000, tv_after=0, tv_every=1, lrate_density=1e-1,
           lrate_k0=1e-1, lrate_rgbnet=1e-3, lrate_decay=20, skip_zero_grad_fields=['density', 'k0'], pg_scale=[])
D, NVOX, STEPSIZE = 128, 256 ** 3, 0.5


def make_model(dev):
    import bench_mpi
    from unboundednerfpytorch_amd.mpi_model import DirectMPIGO
    st = bench_mpi.scene(D, NVOX, STEPSIZE)
    m = DirectMPIGO(xyz_min=[-1.0, -1.0, -1.0], xyz_max=[1.0, 1.0, 1.0], num_voxels=NVOX, mpi_depth=D, fast_color_thres=1e-3,
                    rgbnet_dim=9, rgbnet_depth=3, rgbnet_width=64, viewbase_pe=0)
    assert m.world_size.tolist() == st['world_size'].tolist()
    with torch.no_grad():
        m.density.grid.copy_(st['density_grid'])
        m.act_shift.grid.zero_()                   # (the scene's density already holds a trained geometry)
        m.k0.grid.copy_(st['k0_grid'])
        for lin, w, b in zip((m.rgbnet[0], m.rgbnet[2][0], m.rgbnet[3]), st['rgbnet_weights'], st['rgbnet_biases']):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
        m.mask_cache.mask.copy_(st['mask'])
    return m.to(dev)


def view_rays(dev):
    from unboundednerfpytorch_amd.fourier_render import get_rays_of_a_view
    H, W = 756, 1008
    K = np.array([[820.0, 0, W / 2], [0, 820.0, H / 2], [0, 0, 1]])
    c2w = torch.tensor([[1.0, 0, 0, 0.02], [0, 1.0, 0, -0.01], [0, 0, 1.0, 0.0]], device=dev)
    return [x.reshape(-1, 3).contiguous() for x in get_rays_of_a_view(H, W, K, c2w, ndc=True)]


def _arm(native_step, sync_free=False, **it_kw):
    def set_(m):
        m.fused_forward, m.native_step, m.native_sync_free = True, native_step, sync_free
    return set_, it_kw


NATIVE_ARMS = {"a_fused_op_by_op": _arm(False), "b_native": _arm(True), "c_native_sync_free": _arm(True, True, return_tensors=True)}


def run_native(args, first_step, dev):
    """the three arms of --arms native, alternating step by step on one model and optimizer"""
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model
    m = make_model(dev)
    opt = create_optimizer_or_freeze_model(m, CFG, global_step=0)
    o_all, d_all, v_all = view_rays(dev)
    rk = dict(near=0, far=1, stepsize=STEPSIZE, bg=1, rand_bkgd=True)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    names = list(NATIVE_ARMS)
    ms = {n: [] for n in names}
    for it in range(len(names) * (args.warmup + args.steps)):
        name = names[it % len(names)]
        set_, it_kw = NATIVE_ARMS[name]
        sel = torch.randint(o_all.shape[0], [CFG['N_rand']], device=dev, generator=g)
        o, d, v = o_all[sel], d_all[sel], v_all[sel]
        rgb = torch.rand(CFG['N_rand'], 3, device=dev, generator=g)
        set_(m)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss, psnr = ts.train_iteration(m, opt, o, d, v, rgb, CFG, first_step + it, rk, **it_kw)
        torch.cuda.synchronize()
        if it >= len(names) * args.warmup:
            ms[name].append((time.perf_counter() - t0) * 1e3)
    with torch.no_grad():
        out = m(o, d, v, global_step=1, **rk)
    res = {"workload": "DirectMPIGO train step (llff_default fine stage), native-step arms: world %s, mpi_depth %d, C=9, width 64, %d rays of a "
                       "1008x756 NDC view, stepsize %.1f, TV %s" % (m.world_size.tolist(), D, CFG['N_rand'], STEPSIZE,
                                                                    "dense" if first_step < CFG['tv_dense_before'] else "masked"),
           "samples_per_ray": m.n_samples(STEPSIZE), "survivors_M": int(out["weights"].numel()), "steps_each": args.steps}
    for n in names:
        res[n + "_ms_per_step"] = float(np.median(ms[n]))
        res[n + "_ms_min_max"] = [min(ms[n]), max(ms[n])]
    a = res["a_fused_op_by_op_ms_per_step"]
    res["b_over_a"], res["c_over_a"] = res["b_native_ms_per_step"] / a, res["c_native_sync_free_ms_per_step"] / a
    # the gate: (b) not slower than (a) by more than (a)'s own min-max range in this run
    res["a_range_ms"] = res["a_fused_op_by_op_ms_min_max"][1] - res["a_fused_op_by_op_ms_min_max"][0]
    res["b_within_a_range"] = bool(res["b_native_ms_per_step"] <= a + res["a_range_ms"])
    res["loss"], res["device"] = float(loss), torch.cuda.get_device_name(0)
    return res


def run(args, first_step, dev):
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model
    m = make_model(dev)
    opt = create_optimizer_or_freeze_model(m, CFG, global_step=0)
    o_all, d_all, v_all = view_rays(dev)
    rk = dict(near=0, far=1, stepsize=STEPSIZE, bg=1, rand_bkgd=True)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    ms = {True: [], False: []}
    total = 2 * (args.warmup + args.steps)
    for it in range(total):
        fused = it % 2 == 0
        sel = torch.randint(o_all.shape[0], [CFG['N_rand']], device=dev, generator=g)
        o, d, v = o_all[sel], d_all[sel], v_all[sel]
        rgb = torch.rand(CFG['N_rand'], 3, device=dev, generator=g)
        m.fused_forward, m.native_step = fused, False      # (the fused step of this comparison is the op-by-op one: four autograd nodes)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss, psnr = ts.train_iteration(m, opt, o, d, v, rgb, CFG, first_step + it, rk)
        torch.cuda.synchronize()
        if it >= 2 * args.warmup:
            ms[fused].append((time.perf_counter() - t0) * 1e3)
    with torch.no_grad():
        m.fused_forward = True
        out = m(o, d, v, global_step=1, **rk)
    f, c = float(np.median(ms[True])), float(np.median(ms[False]))
    return {"workload": "DirectMPIGO train step (llff_default fine stage): world %s, mpi_depth %d, C=9, width 64, %d rays of a 1008x756 NDC "
                        "view, stepsize %.1f, TV %s" % (m.world_size.tolist(), D, CFG['N_rand'], STEPSIZE,
                                                       "dense" if first_step < CFG['tv_dense_before'] else "masked"),
            "samples_per_ray": m.n_samples(STEPSIZE), "survivors_M": int(out["weights"].numel()), "steps_each": args.steps,
            "fused_ms_per_step": f, "op_by_op_ms_per_step": c, "ratio": c / f,
            "fused_ms_min_max": [min(ms[True]), max(ms[True])], "op_by_op_ms_min_max": [min(ms[False]), max(ms[False])],
            "loss": float(loss), "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="timed steps of EACH variant (alternating)")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--phase", default="both")
    ap.add_argument("--arms", default="fused", choices=["fused", "native"], help="fused vs op-by-op chain | the three native-step arms")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mpi", "bench_mpi_train_native.txt" if args.arms == "native" else "bench_mpi_train.txt")
    assert args.steps >= 20, "median of at least 20 steps"
    dev = torch.device("cuda", 0)
    lines = []
    for first in {"dense": [1], "masked": [10001]}.get(args.phase, [1, 10001]):
        lines.append(json.dumps((run_native if args.arms == "native" else run)(args, first, dev)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
