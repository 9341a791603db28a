"""run_render.render_video (8-bit frames made on the device, csrc/ugrid_video.hip) against the parent's path for the same output,
on one MI355X: run_render.render_viewpoints followed by the host expressions of the reference's render program
(FourierGrid/run_render.py:284, :307, :308-315) restated in numpy (tests/video_cases.py; video.rainbow_table() for the colour map).

  scenes   the 800 x 800 DirectVoxGO scene of tools/bench_dvgo.py with --views-dvgo views (64) and a 1920 x 1080 FourierGrid scene
           (bench.py's trained-like S1b statistics at --fg-grid^3) with --views-fg views (16);
  modes    rgb only, depth='max', depth='percentile' (unrotated frames: the common case);
  clock    host clock around a whole call; both calls end with their arrays on the host behind a device synchronise.  Both arms
           alternate in ONE process after a warm-up call each; a figure is the median of --blocks blocks with min and max;
  bytes    the two arms' uint8 outputs are compared byte for byte in the same run;
  kernels  ugrid_frame_rgb8 (k = 0 and k = 1, with and without the db / dmax outputs), ugrid_depth8_max, ugrid_depth8_map with device
           events around blocks of --iters launches, ugrid_depthvis_select (it synchronises: host clock) on random frames of both sizes.

The board's state is recorded before and after.  No threshold is applied: the table says what came out.

    python tools/bench_video.py [--out profiles/video/video.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import board_state  # noqa: E402
import video_cases as vc  # noqa: E402
from bench_tensorf import ab  # noqa: E402

MODES = (None, "max", "percentile")


def host_video(rgbs, depths, bgmaps, mode, table):
    """the reference's host lines on render_viewpoints' stacks"""
    rgb8 = vc.to8b(rgbs)                                                              # :261 / :283 / :307
    if mode is None:
        return rgb8, None
    if mode == "max":
        return rgb8, vc.to8b(1 - depths / np.max(depths))                             # :284
    depths_vis = depths * (1-bgmaps) + bgmaps                                         # :308
    mask = bgmaps < 0.1
    if not mask.max():
        return rgb8, None
    dmin, dmax = np.percentile(depths_vis[bgmaps < 0.1], q=[5, 95])                   # :313
    x = 1 - np.clip((depths_vis - dmin) / (dmax - dmin), 0, 1)                        # :314, the colour map as its table
    return rgb8, vc.lookup(table, x).squeeze()


def dvgo_scene(dev, n_views):
    from bench_dvgo import make_dvgo_state
    from unboundednerfpytorch_amd.dvgo_render import DirectVoxGORenderer
    H = W = 800
    rend = DirectVoxGORenderer(make_dvgo_state(160, dev), dev)
    f = 1111.1 * W / 800.0
    K = [[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]]
    base = np.array([[-0.9999, 0.0042, -0.0133, -0.0538], [-0.0140, -0.2997, 0.9539, 3.8455], [0.0, 0.9540, 0.2997, 1.2081]], dtype=np.float32)
    poses = []
    for i in range(n_views):
        p = base.copy()
        p[:, 3] += np.array([0.01 * i, -0.01 * i, 0.005 * i], dtype=np.float32) * (16.0 / max(n_views, 16))
        poses.append(p)
    return rend, poses, [(H, W)] * n_views, [K] * n_views, dict(near=2.0, far=6.0, stepsize=0.5, bg=1)


def fourier_scene(dev, n_views, G):
    import bench
    from unboundednerfpytorch_amd.fourier_render import FourierGridRenderer
    H, W = 1080, 1920
    rend = FourierGridRenderer(bench.make_state_surfaces(G, dev, 0), dev)
    f = 0.5 * W / np.tan(0.5 * np.deg2rad(60.0))
    K = [[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]]
    poses = [bench.camera(0.25 * i, "cpu").numpy().astype(np.float32) for i in range(n_views)]
    return rend, poses, [(H, W)] * n_views, [K] * n_views, dict(stepsize=0.5)


def scene_case(name, scene, blocks):
    from unboundednerfpytorch_amd import video
    from unboundednerfpytorch_amd.run_render import render_video, render_viewpoints
    rend, poses, HW, Ks, kw = scene
    n = len(poses)
    table = video.rainbow_table()
    out = {"H": HW[0][0], "W": HW[0][1], "views": n, "frames_in_flight": int(getattr(rend, "frames_in_flight", 2)),
           "clock": "host, around the whole call (arrays on the host, device synchronised)", "modes": {}}

    def parent(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rgbs, depths, bgmaps = render_viewpoints(rend, poses, HW, Ks, kw)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        res = host_video(rgbs, depths, bgmaps, mode, table)
        return (time.perf_counter() - t0) * 1e3 / n, (t1 - t0) * 1e3 / n, res

    def device(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rgb8, depth8, info = render_video(rend, poses, HW, Ks, kw, depth=mode)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n, (rgb8, depth8), info

    for mode in MODES:
        p, d = parent(mode), device(mode)                    # warm-up of both arms, and the byte comparison
        same_rgb = bool(np.array_equal(p[2][0], d[1][0]))
        same_depth = (p[2][1] is None and d[1][1] is None) or bool(p[2][1] is not None and d[1][1] is not None and np.array_equal(p[2][1], d[1][1]))
        info = d[2]
        del p, d
        t = {"render_viewpoints_plus_numpy": [], "render_viewpoints_alone": [], "render_video": []}
        for _ in range(blocks):
            a = parent(mode)
            t["render_viewpoints_plus_numpy"].append(a[0])
            t["render_viewpoints_alone"].append(a[1])
            del a
            t["render_video"].append(device(mode)[0])
        r = {k: {"median_ms_per_view": statistics.median(v), "min": min(v), "max": max(v), "blocks": len(v)} for k, v in t.items()}
        r.update(rgb8_identical=same_rgb, depth8_identical=bool(same_depth), info={k: (None if v is None else float(v)) for k, v in info.items()})
        out["modes"][str(mode)] = r
        print("%s %-10s per view: parent %.3f ms (render_viewpoints alone %.3f), render_video %.3f ms; rgb8 identical %s, depth8 identical %s" % (
            name, mode, r["render_viewpoints_plus_numpy"]["median_ms_per_view"], r["render_viewpoints_alone"]["median_ms_per_view"],
            r["render_video"]["median_ms_per_view"], same_rgb, same_depth), flush=True)
    return out


def kernel_case(H, W, dev, iters, blocks):
    from unboundednerfpytorch_amd import video
    n = H * W
    frame = torch.rand(n, 5, device=dev)
    frame[:, 3] *= 40.0
    out3, out1 = torch.empty(n * 3, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    db = torch.empty(n, 2, device=dev)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    table = torch.from_numpy(video.rainbow_table()).to(dev)
    video.frame_rgb8(frame, H, W, out=out3, db=db)
    arms = {"frame_rgb8_k0": lambda: video.frame_rgb8(frame, H, W, False, 0, out=out3),
            "frame_rgb8_k1": lambda: video.frame_rgb8(frame, H, W, False, 1, out=out3),
            "frame_rgb8_k0_db_dmax": lambda: video.frame_rgb8(frame, H, W, False, 0, out=out3, db=db, dmax=word),
            "frame_rgb8_k0_db": lambda: video.frame_rgb8(frame, H, W, False, 0, out=out3, db=db),
            "frame_rgb8_k0_dmax": lambda: video.frame_rgb8(frame, H, W, False, 0, out=out3, dmax=word),
            "frame_rgb8_k1_db_dmax": lambda: video.frame_rgb8(frame, H, W, False, 1, out=out3, db=db, dmax=word),
            "depth8_max_k0": lambda: video.depth8_max(db, H, W, 40.0, False, 0, out=out1),
            "depth8_max_k1": lambda: video.depth8_max(db, H, W, 40.0, False, 1, out=out1),
            "depth8_map_k0": lambda: video.depth8_map(db, H, W, 2.0, 38.0, table, False, 0, out=out3),
            "depth8_map_k1": lambda: video.depth8_map(db, H, W, 2.0, 38.0, table, False, 1, out=out3)}
    r = ab(arms, iters, blocks)
    moved = {"frame_rgb8_k0": 23, "frame_rgb8_k1": 23, "frame_rgb8_k0_db_dmax": 31, "frame_rgb8_k1_db_dmax": 31, "frame_rgb8_k0_db": 31, "frame_rgb8_k0_dmax": 23, "depth8_max_k0": 9,
             "depth8_max_k1": 9, "depth8_map_k0": 11, "depth8_map_k1": 11}       # bytes a pixel read + written (the rgb8 kernels fetch whole 20-byte rows)
    for k, v in r.items():
        v["GB_per_s"] = moved[k] * n / (v["median_ms"] * 1e-3) / 1e9
    # the select synchronises the stream: host clock, the whole call (count + four ranks: three passes)
    db16 = torch.rand(16 * n, 2, device=dev)
    db16[:, 1] *= 0.2
    cnt = video.depthvis_select(db16, ())[0]
    ranks = sorted({int((cnt - 1) * 0.05), int((cnt - 1) * 0.05) + 1, int((cnt - 1) * 0.95), int((cnt - 1) * 0.95) + 1})
    ts = []
    for _ in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        video.depthvis_select(db16, ranks)
        ts.append((time.perf_counter() - t0) * 1e3)
    r["depthvis_select_16_frames_4_ranks"] = {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "blocks": blocks, "pixels": 16 * n,
                                              "taking_part": cnt, "clock": "host (the call synchronises its stream three times)"}
    r.update(H=H, W=W)
    for k, v in r.items():
        if isinstance(v, dict):
            print("kernel %dx%d %-34s %.4f ms (%.4f - %.4f)%s" % (H, W, k, v["median_ms"], v["min_ms"], v["max_ms"],
                                                                  "  %.0f GB/s" % v["GB_per_s"] if "GB_per_s" in v else ""), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--views-dvgo", type=int, default=64)
    ap.add_argument("--views-fg", type=int, default=16)
    ap.add_argument("--fg-grid", type=int, default=128)
    ap.add_argument("--skip-scenes", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU (no fallback)"
    assert a.blocks >= 5
    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    res = {"device": torch.cuda.get_device_name(dev), "board_before": board_state.snapshot(), "numpy": np.__version__,
           "note": "one device; both arms alternate in one process; medians of blocks with min / max; host clock around calls that end in a "
                   "device synchronise; kernel times from device events around blocks of launches"}
    res["kernels"] = [kernel_case(H, W, dev, a.iters, a.blocks) for H, W in ((800, 800), (1080, 1920))]
    if not a.skip_scenes:
        res["dvgo_800"] = scene_case("dvgo_800", dvgo_scene(dev, a.views_dvgo), a.blocks)
        torch.cuda.empty_cache()
        res["fourier_1080p"] = scene_case("fourier_1080p", fourier_scene(dev, a.views_fg, a.fg_grid), a.blocks)
        res["fourier_1080p"]["grid"] = a.fg_grid
    res["board_after"] = board_state.snapshot()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
