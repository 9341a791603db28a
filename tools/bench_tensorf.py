"""TensoRF kernels against the torch composition of the reference's formula, at configs/nerf/ship.tensorf.py's final shape: world 384^3;
density R = 8, C = 1, ~1 M points; k0 R = 24, C = 12, ~150 k points; points uniform in the box, from a seed.

Timed: the query forward, forward + backward, the TV launch, the bake.  Arms: "hip" = csrc/ugrid_tensorf.hip through
grid.TensoRFQuery / tensorf_tv_add_grad / tensorf_bake; "torch" = grid.tensorf_compose (six grid_sample calls, cat, mm; autograd for
the backward), the reference's smooth-L1 TV loss + backward, and the reference's einsum bake at the largest world whose [rows, X, Y, Z]
intermediate fits (--bake-world, default 128).  Both arms run in ONE process, alternating, after a warm-up; each arm's figure is the
median of --blocks equal blocks of --iters launches.  The board's state is recorded before and after.

    python tools/bench_tensorf.py [--out profiles/tensorf/query.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import board_state  # noqa: E402
from unboundednerfpytorch_amd import grid  # noqa: E402


def block_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def ab(arms, iters, blocks, warmup=3):
    """arms: {name: fn}; alternating blocks in one process -> {name: {median_ms, min_ms, max_ms, blocks}}"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(blocks):
        for k, fn in arms.items():
            t[k].append(block_ms(fn, iters))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "blocks": len(v), "iters_per_block": iters} for k, v in t.items()}


def make(world, R, C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    X, Y, Z = world
    shp = [(1, R, X, Y), (1, R, X, Z), (1, R, Y, Z), (1, R, X, 1), (1, R, Y, 1), (1, R, Z, 1)]
    canon = [(torch.randn(s, generator=g) * 0.1).to(dev) for s in shp]
    f_vec = (torch.rand(3 * R, C, generator=g) - 0.5).to(dev) if C > 1 else None
    return canon, f_vec


def tv_torch(params, w):
    xy, xz, yz, xv, yv, zv = params
    s = lambda a, b: F.smooth_l1_loss(a, b, reduction='sum')
    loss = w[0] * s(xy[:, :, 1:], xy[:, :, :-1]) + w[1] * s(xy[:, :, :, 1:], xy[:, :, :, :-1]) + w[0] * s(xz[:, :, 1:], xz[:, :, :-1]) \
        + w[2] * s(xz[:, :, :, 1:], xz[:, :, :, :-1]) + w[1] * s(yz[:, :, 1:], yz[:, :, :-1]) + w[2] * s(yz[:, :, :, 1:], yz[:, :, :, :-1]) \
        + w[0] * s(xv[:, :, 1:], xv[:, :, :-1]) + w[1] * s(yv[:, :, 1:], yv[:, :, :-1]) + w[2] * s(zv[:, :, 1:], zv[:, :, :-1])
    (loss / 6).backward()


def bake_torch(params, f_vec):
    xy, xz, yz, xv, yv, zv = [p[0] for p in params]
    if f_vec is None:
        return (torch.einsum('rxy,rz->xyz', xy, zv[:, :, 0]) + torch.einsum('rxz,ry->xyz', xz, yv[:, :, 0]) + torch.einsum('ryz,rx->xyz', yz, xv[:, :, 0]))[None, None]
    feat = torch.cat([torch.einsum('rxy,rz->rxyz', xy, zv[:, :, 0]), torch.einsum('rxz,ry->rxyz', xz, yv[:, :, 0]),
                      torch.einsum('ryz,rx->rxyz', yz, xv[:, :, 0])])
    return torch.einsum('rxyz,rc->cxyz', feat, f_vec)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=384)
    ap.add_argument("--bake-world", type=int, default=128)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lo, hi = torch.tensor([-1.0, -1.0, -1.0], device=dev), torch.tensor([1.0, 1.0, 1.0], device=dev)
    res = {"world": a.world, "board_before": board_state.snapshot(), "cases": {}}
    for name, R, C, n in (("density", 8, 1, 1_000_000), ("k0", 24, 12, 150_000)):
        canon, f_vec = make((a.world,) * 3, R, C, dev, 7)
        pts = (torch.rand(n, 3, generator=torch.Generator().manual_seed(11)) * 2 - 1).to(dev)
        go = torch.randn((n, C) if C > 1 else (n,), generator=torch.Generator().manual_seed(12)).to(dev)
        case = {"R": R, "C": C, "points": n}
        for layout in ("complast", "canonical"):
            st = [t.contiguous(memory_format=torch.channels_last) if layout == "complast" else t for t in canon]
            leaves = [t.clone().requires_grad_(True) for t in st]
            fl = f_vec.clone().requires_grad_(True) if f_vec is not None else None
            cl = [t.clone().requires_grad_(True) for t in canon]
            cfl = f_vec.clone().requires_grad_(True) if f_vec is not None else None

            def hip_fwd():
                with torch.no_grad():
                    return grid.tensorf_query(st, f_vec, pts, lo, hi)

            def torch_fwd():
                with torch.no_grad():
                    return grid.tensorf_compose(canon, f_vec, pts, lo, hi)

            def hip_fb():
                for t in leaves + ([fl] if fl is not None else []):
                    t.grad = None
                (grid.TensoRFQuery.apply(pts, lo, hi, *leaves, fl) * go).sum().backward()

            def torch_fb():
                for t in cl + ([cfl] if cfl is not None else []):
                    t.grad = None
                (grid.tensorf_compose(cl, cfl, pts, lo, hi) * go).sum().backward()
            grads = [torch.zeros_like(t, memory_format=torch.preserve_format) for t in st]

            def hip_tv():
                grid.tensorf_tv_add_grad(st, grads, 0.1, 0.1, 0.1)

            def torch_tv():
                for t in cl:
                    t.grad = None
                tv_torch(cl, (0.1, 0.1, 0.1))
            case[layout] = {"forward": ab({"hip": hip_fwd, "torch": torch_fwd}, a.iters, a.blocks),
                            "forward_backward": ab({"hip": hip_fb, "torch": torch_fb}, a.iters, a.blocks),
                            "tv": ab({"hip": hip_tv, "torch": torch_tv}, a.iters, a.blocks)}
            d = float((hip_fwd() - torch_fwd()).abs().max())
            case[layout]["max_abs_diff_hip_vs_torch_forward"] = d
            del leaves, cl, grads
        # the bake: the kernel at the full world, both factor layouts (no baseline fits there for C > 1: the einsum's [rows, X, Y, Z]
        # intermediate), and kernel against baseline at --bake-world.  The kernel writes a preallocated output; the baseline is
        # the reference's get_dense_grid as it stands (grid.py:156-169: for C == 1 three einsums and two additions, for C > 1 the
        # concatenated [rows, X, Y, Z] features and one more einsum), which allocates its result and intermediates itself.
        st = [t.contiguous(memory_format=torch.channels_last) for t in canon]
        full = grid.tensorf_bake(canon, f_vec)
        case["bake_full_world"] = ab({"hip": lambda: grid.tensorf_bake(canon, f_vec, out=full)}, 2, 3, warmup=1)
        case["bake_full_world_complast"] = ab({"hip": lambda: grid.tensorf_bake(st, f_vec, out=full)}, 2, 3, warmup=1)
        case["bake_full_world"]["output_bytes"] = 4 * C * a.world ** 3
        del full
        small, fs = make((a.bake_world,) * 3, R, C, dev, 8)
        ss = small
        sout = grid.tensorf_bake(ss, fs)
        case["bake_at_%d" % a.bake_world] = ab({"hip": lambda: grid.tensorf_bake(ss, fs, out=sout), "torch": lambda: bake_torch(small, fs)}, 2, a.blocks, warmup=1)
        case["bake_at_%d" % a.bake_world]["torch_intermediate_bytes"] = 4 * 3 * R * a.bake_world ** 3 if C > 1 else 0
        res["cases"][name] = case
        del canon, st, small, ss
        torch.cuda.empty_cache()
    res["board_after"] = board_state.snapshot()
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    for name, case in res["cases"].items():
        for layout in ("complast", "canonical"):
            for what, r in case[layout].items():
                if isinstance(r, dict):
                    print("%s %s %s: hip %.3f ms, torch %.3f ms" % (name, layout, what, r["hip"]["median_ms"], r["torch"]["median_ms"]))
        for k in case:
            if k.startswith("bake"):
                print(name, k, {arm: round(v["median_ms"], 3) for arm, v in case[k].items() if isinstance(v, dict)})


if __name__ == "__main__":
    main()
