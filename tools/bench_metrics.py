"""Frame metrics on one MI355X: ugrid_frame_metrics (squared-error sum + SSIM map sum, csrc/ugrid_metrics.hip) on a 1920 x 1080
frame read as the rgb columns of a packed [H*W,5] render result against an [H*W,3] ground truth -- the frame loop's call.
HIP events around each call (both kernels of the entry point), a warm-up, then --reps calls; the host time is that of the
numpy fp64 implementation of tests/metrics_cases.py for one frame on the same machine.  Prints one JSON line.

    python tools/bench_metrics.py [--reps 50] [--warmup 5] [--no-host]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy timing (seconds per frame)")
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20")
    from unboundednerfpytorch_amd import metrics
    import metrics_cases
    H, W = a.height, a.width
    rs = np.random.RandomState(0)
    img = rs.rand(H, W, 3).astype(np.float32)
    gt = np.clip(img + 0.05 * rs.randn(H, W, 3), 0.0, 1.0).astype(np.float32)
    packed = torch.zeros(H * W, 5, device="cuda")
    packed[:, :3] = torch.from_numpy(img).cuda().reshape(-1, 3)
    g = torch.from_numpy(gt).cuda().reshape(-1, 3)
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    ws = torch.empty(metrics.workspace_bytes(H, W), dtype=torch.uint8, device="cuda")
    for _ in range(a.warmup):
        metrics.frame_metrics(packed, g, H=H, W=W, out=out, ws=ws)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
    for s, e in ev:
        s.record()
        metrics.frame_metrics(packed, g, H=H, W=W, out=out, ws=ws)
        e.record()
    torch.cuda.synchronize()
    ms = sorted(s.elapsed_time(e) for s, e in ev)
    sums = out.cpu().numpy()
    res = {"bench": "frame_metrics", "H": H, "W": W, "reps": a.reps, "warmup": a.warmup,
           "kernel_ms_median": ms[len(ms) // 2], "kernel_ms_min": ms[0], "kernel_ms_max": ms[-1],
           "ssim": metrics.mean_ssim(sums[1], H, W), "psnr": float(metrics.psnr_from_sums(sums, H, W)),
           "device": torch.cuda.get_device_name(0)}
    if not a.no_host:
        t0 = time.perf_counter()
        m = metrics_cases.ssim_map_numpy(img, gt)
        res["host_numpy_s"] = time.perf_counter() - t0
        res["ssim_abs_diff_vs_numpy"] = abs(res["ssim"] - float(m.mean()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
