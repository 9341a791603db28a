"""The frame epilogue kernels of csrc/ugrid_frame.hip against the torch compositions they replace, on one MI355X:

  epilogue   ugrid_frame_assemble from the three per-ray arrays  vs  untile x 3 + cat (run_render._render_packed with
             FUSED_ASSEMBLY False), at 1920 x 1080 and 800 x 800;
  gathered   ugrid_frame_assemble from a gathered buffer in the world-8 layout (bands, block rows)  vs  index_select with a
             resident int64 index (bench.py's FrameBench._assemble);
  pack       ugrid_frame_pack  vs  zeros + three strided copies (dist.render_sharded), a rank's share of a 1080p frame at world 8;
  views      run_render.render_viewpoints per view with FUSED_ASSEMBLY on and off, the 800 x 800 DirectVoxGO shape of
             tools/bench_dvgo.py (host clock around the whole call, which ends with every frame on the host).

Both arms of a comparison alternate in ONE process after a warm-up; a figure is the median of --blocks equal blocks (min and max
beside it), device events around a block.  Random payloads.  The board's state is recorded before and after.  Ranks sharing one
device say nothing about scaling: nothing here runs on more than one device.

    python tools/bench_frame_pipeline.py [--out profiles/frame_pipeline/assemble.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import board_state  # noqa: E402
from bench_tensorf import ab  # noqa: E402


def epilogue_case(H, W, dev, iters, blocks):
    from unboundednerfpytorch_amd.dist import FramePlan, frame_assemble
    from unboundednerfpytorch_amd.fourier_render import untile
    R = H * W
    rgb, depth, last = torch.rand(R, 3, device=dev), torch.rand(R, device=dev), torch.rand(R, device=dev)
    plan = FramePlan(H, W, 1)
    assert plan.tile8

    def parent():
        a, b, c = untile(rgb, H, W), untile(depth, H, W), untile(last, H, W)
        return torch.cat([a.reshape(-1, 3), b.reshape(-1, 1), c.reshape(-1, 1)], dim=1).reshape(-1)

    def fused():
        return frame_assemble(plan, rgb=rgb, depth=depth, last=last).reshape(-1)
    same = bool(torch.equal(parent().view(torch.int32), fused().view(torch.int32)))
    r = ab({"untile_x3_cat": parent, "frame_assemble": fused}, iters, blocks)
    r.update(H=H, W=W, bit_identical=same, payload_bytes=R * 20, bytes_moved_fused=2 * R * 20)
    return r


def gathered_case(H, W, world, deal, dev, iters, blocks):
    from unboundednerfpytorch_amd.dist import FramePlan, frame_assemble
    plan = FramePlan(H, W, world, deal)
    full = torch.rand(world * plan.per, 5, device=dev)
    idx = plan.src_index().to(dev)
    same = bool(torch.equal(torch.index_select(full, 0, idx).view(torch.int32), frame_assemble(plan, gathered=full).view(torch.int32)))
    r = ab({"index_select": lambda: torch.index_select(full, 0, idx), "frame_assemble": lambda: frame_assemble(plan, gathered=full)}, iters, blocks)
    r.update(H=H, W=W, world=world, deal=deal, deal_group=plan.deal_group, per=plan.per, bit_identical=same, payload_bytes=H * W * 20,
             index_bytes=H * W * 8)
    return r


def pack_case(H, W, world, dev, iters, blocks):
    from unboundednerfpytorch_amd.dist import FramePlan, frame_pack
    plan = FramePlan(H, W, world)
    n = plan.px(world - 1).numel()           # the last rank's band is the short one: rows n..per are zero-filled
    rgb, depth, last = torch.rand(n, 3, device=dev), torch.rand(n, device=dev), torch.rand(n, device=dev)

    def parent():
        tile = torch.zeros(plan.per, 5, dtype=torch.float32, device=dev)
        tile[:n, 0:3] = rgb
        tile[:n, 3] = depth
        tile[:n, 4] = last
        return tile
    same = bool(torch.equal(parent().view(torch.int32), frame_pack(rgb, depth, last, plan.per).view(torch.int32)))
    r = ab({"zeros_3_copies": parent, "frame_pack": lambda: frame_pack(rgb, depth, last, plan.per)}, iters, blocks)
    r.update(H=H, W=W, world=world, n=n, per=plan.per, bit_identical=same)
    return r


def views_case(dev, n_views, blocks):
    import numpy as np
    from bench_dvgo import make_dvgo_state
    from unboundednerfpytorch_amd import run_render
    from unboundednerfpytorch_amd.dvgo_render import DirectVoxGORenderer
    H = W = 800
    rend = DirectVoxGORenderer(make_dvgo_state(160, dev), dev)
    f = 1111.1 * W / 800.0
    K = [[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]]
    base = np.array([[-0.9999, 0.0042, -0.0133, -0.0538], [-0.0140, -0.2997, 0.9539, 3.8455], [0.0, 0.9540, 0.2997, 1.2081]], dtype=np.float32)
    poses = []
    for i in range(n_views):
        p = base.copy()
        p[:, 3] += np.array([0.01 * i, -0.01 * i, 0.005 * i], dtype=np.float32)
        poses.append(p)
    kw = dict(near=2.0, far=6.0, stepsize=0.5, bg=1)
    saved = run_render.FUSED_ASSEMBLY

    def run(fused):
        run_render.FUSED_ASSEMBLY = fused
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run_render.render_viewpoints(rend, poses, [(H, W)] * n_views, [K] * n_views, kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n_views, out
    try:
        a, b = run(True)[1], run(False)[1]
        same = all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
        run(True), run(False)
        t = {"untile_x3_cat": [], "frame_assemble": []}
        for _ in range(blocks):
            t["untile_x3_cat"].append(run(False)[0])
            t["frame_assemble"].append(run(True)[0])
    finally:
        run_render.FUSED_ASSEMBLY = saved
    r = {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "blocks": len(v), "views_per_block": n_views} for k, v in t.items()}
    r.update(H=H, W=W, frames_in_flight=int(rend.frames_in_flight), bit_identical=bool(same), clock="host, around render_viewpoints (frames on the host)")
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--skip-views", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU (no fallback)"
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    res = {"device": torch.cuda.get_device_name(dev), "board_before": board_state.snapshot(),
           "note": "one device; both arms alternate in one process; medians of blocks with min / max; no run on more than one device exists"}
    res["epilogue"] = [epilogue_case(H, W, dev, a.iters, a.blocks) for H, W in ((1080, 1920), (800, 800))]
    res["gathered"] = [gathered_case(1080, 1920, 8, deal, dev, a.iters, a.blocks) for deal in ("bands", "rows")]
    res["pack"] = [pack_case(1080, 1920, 8, dev, a.iters, a.blocks)]
    if not a.skip_views:
        res["render_viewpoints_dvgo_800"] = views_case(dev, a.views, a.blocks)
        v = res["render_viewpoints_dvgo_800"]
        spread = v["untile_x3_cat"]["max_ms"] - v["untile_x3_cat"]["min_ms"]
        # the rule FUSED_ASSEMBLY's default follows: on unless slower than the parent's epilogue by more than that arm's own spread
        v["fused_default_rule"] = {"parent_spread_ms": spread, "fused_minus_parent_ms": v["frame_assemble"]["median_ms"] - v["untile_x3_cat"]["median_ms"],
                                   "default_true": bool(v["frame_assemble"]["median_ms"] - v["untile_x3_cat"]["median_ms"] <= spread)}
    res["board_after"] = board_state.snapshot()
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    for name in ("epilogue", "gathered", "pack"):
        for c in res[name]:
            arms = [k for k in c if isinstance(c[k], dict) and "median_ms" in c[k]]
            print(name, {k: c[k] for k in ("H", "W", "deal") if k in c}, "bit-identical:", c["bit_identical"],
                  "; ".join("%s %.4f ms (%.4f - %.4f)" % (k, c[k]["median_ms"], c[k]["min_ms"], c[k]["max_ms"]) for k in arms))
    if not a.skip_views:
        v = res["render_viewpoints_dvgo_800"]
        print("render_viewpoints 800 x 800 DirectVoxGO, per view:", "; ".join("%s %.4f ms (%.4f - %.4f)" % (k, v[k]["median_ms"], v[k]["min_ms"], v[k]["max_ms"])
                                                                              for k in ("untile_x3_cat", "frame_assemble")), v["fused_default_rule"])


if __name__ == "__main__":
    main()
