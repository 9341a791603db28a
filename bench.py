#!/usr/bin/env python
"""bench.py -- headline benchmark of the MI355X FourierGrid render path (BASELINE.json metric).

Workload (SURVEY.md section 8d "S1", BASELINE.json configs[1]): one synthetic Mip-NeRF-360-'garden'-shaped
frame -- 1920x1080 rays x 256 samples/ray through a FourierGridModel with G=200^3 voxels, F=3 (P=7 Fourier
levels), C=12 feature channels, rgbnet 39->128->128->3, contracted unbounded scene, stepsize 1.31,
fast_color_thres 1e-4.  A "step" = one full frame: ray generation + ray march (density query + alpha + compositing
scan) + shade (k0 query + rgbnet + weighted sum); grids and camera are resident in HBM.

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]      (N>1: launched by torch.distributed.run)

Prints ONE JSON line on rank 0.  value = Msamples/s = R * S / t_step (all generated samples, before thresholding).
A plain run sets up, warms up, times the K steps and prints the line (metric, value, unit, ms_per_step, ...); --dump-outputs
DIR also writes the frame of the last timed step as DIR/<output>.npy.  Everything else -- the per-kernel one-stream region,
roofline, CPU baseline and parity, scaling proxy, weak scaling, the secondary scenes and training steps, the detail file --
runs only with --full.
Multi-GPU is STRONG-scaled: the N ranks render ONE frame -- rank r takes a contiguous band of the frame's 64-ray tiles (--deal rows /
tiles: block rows or single tiles dealt round-robin) and the rendered tiles [R/N,5] are exchanged with one RCCL all-gather inside the timed step
(issued asynchronously: frame k's exchange overlaps frame k+1's render; the last one is waited for before the closing
barrier).  A short weak-scaled loop (every rank its own full frame) is reported beside it as `weak_scaling`.
A second scene (`secondary`, S1b: smooth density with surfaces, ~half of the rays terminate early) shows what wave-level
early termination buys and carries its own parity numbers.
"""
import argparse
import hashlib
import json
import math
import os
import sys
import time

os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")      # (unboundednerfpytorch_amd/__init__.py: a hardware queue per stream in flight; before the runtime starts)
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# peaks used by the roofline block (/opt/skills/guides/MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0               # HBM3E spec peak (~6.3 TB/s achievable)
N_CU, N_SIMD, CLK_HZ = 256, 1024, 2.4e9
L1_PEAK_GBS = N_CU * 64 * CLK_HZ / 1e9          # vector L1 / texture path, NOMINAL: 64 B per clock per CU = 39.3 TB/s
# ... and as MEASURED on an MI355X by tools/microbench/l1_dwordx4.hip (pure L1-hit global_load_dwordx4 stream on every CU;
# profiles/r03/microbench_l1_dwordx4.json); None until that file exists
PROFILE_DIR = os.path.join(ROOT, "profiles", "r06")        # this round's counters; older rounds' files are used only when they were
PROFILE_FALLBACK = ("r05",)                                # taken on the SAME device code (the hash check below decides)
MFMA_F16_PEAK_TFLOPS = 2500.0       # dense f16/bf16 MFMA peak
VALU_PEAK_GINST = N_SIMD * CLK_HZ / 2 / 1e9     # one wave64 VALU instruction per 2 cycles per SIMD

# S1 scene statistics (white-noise grids; calibrated with the CPU oracle so that ~5% of samples survive both
# thresholds, tools/calibrate_s1.py)
DENS_MEAN, DENS_STD = -8.5, 24.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--grid", type=int, default=200)
    ap.add_argument("--scene", default="s1", choices=["s1", "s1b"], help="headline scene (s1b is also run as `secondary`)")
    ap.add_argument("--freq", type=int, default=3, help="fourier_freq_num F of the scene (P = 1 + 2F levels); 4 with --scene s1b --stepsize 0.5 = "
                    "truck_single.py's shape (BASELINE configs[2]), which the default run times as `secondary_truck_render`")
    ap.add_argument("--no-truck", action="store_true", help="skip the truck-shaped secondary render (F = 4, P = 9, S = 668; 30 GB of bricks)")
    ap.add_argument("--no-secondary", action="store_true", help="skip the S1b secondary scene")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--deal", default="bands", choices=["bands", "rows", "tiles"],
                    help="N>1: how the frame's 64-ray tiles (8x8 pixel blocks, in block-row order) are split over the ranks: contiguous "
                    "BANDS (default: SURVEY 8e's partition; on the S1 frame the best of the three in `scaling_proxy`: 6.25 x predicted at "
                    "N = 8 against 5.8 x, every rank keeps its neighbours' cells), whole block ROWS of the image dealt round-robin "
                    "(balanced on scenes with sky, keeps horizontal neighbours) or single TILES dealt round-robin (finest balance, "
                    "least sharing); --deal-group K deals groups of K tiles")
    ap.add_argument("--contiguous", action="store_true", help="(= --deal bands; kept for older command lines)")
    ap.add_argument("--deal-group", type=int, default=0, help="N>1: deal groups of this many consecutive tiles round-robin (overrides --deal)")
    ap.add_argument("--no-proxy", action="store_true", help="skip `scaling_proxy` (every rank's share of an N-way deal rendered ALONE on this GPU)")
    ap.add_argument("--mlp-mode", type=int, default=None, help="rgbnet arithmetic: 0 fp32 MFMA, 1 bf16x3, 2 fp16x2 (default: what ugrid_pack_mlp reports usable)")
    ap.add_argument("--pipeline", type=int, default=0, help="ray chunks software-pipelined over two streams (0 = off)")
    ap.add_argument("--frame-pair", type=int, default=-1, help="consecutive frames alternate between two streams, each with a work list of its own: "
                    "the march of frame k+1 runs beside the shade of frame k (a 1/N share alone fills 0.66 of a wave per slot and stages 93 KB "
                    "of weights per shade launch; whole frames: 8.75 -> 8.40 ms on S1, 13.98 -> 12.68 ms on the truck shape, frames bit-identical, "
                    "profiles/r06/frame_pair_n1.txt).  -1 / 1 = on (the per-kernel durations then come from a second, one-stream timed region), 0 = one stream")
    ap.add_argument("--frames-in-flight", type=int, default=3, help="streams / work lists the frames take in turn when --frame-pair is on (3: 2 % faster than 2 on "
                    "S1, S1b at S = 668 and the truck shape, three repetitions each on two boards; 4 is no better: profiles/r06/frames_in_flight_sweep.txt)")
    ap.add_argument("--tune", action="append", default=[], help="key=value speed knob (ugrid_tune), repeatable")
    ap.add_argument("--shuffle-rays", action="store_true", help="render the frame's rays in a random order (incoherent 64-ray tiles, "
                    "like a training batch): shows what the kernels owe to neighbouring pixels sharing cells")
    ap.add_argument("--ray-tile", type=int, default=8, help="the frame's rays are rendered in T x T pixel blocks (one march wave = "
                    "one 8x8 block, fourier_render.pixel_tile_order -- what render_view does); 0 = 64-pixel row segments")
    ap.add_argument("--stepsize", type=float, default=None, help="sampling step in voxels (default 1.31 at G = 200: the 256-sample frame of the metric; "
                    "0.5 = garden_single.py's own sampling, S = 668)")
    ap.add_argument("--cpu-chunks", type=int, default=12, help="8192-ray chunks timed for the CPU baseline (~1 s each)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write the frame the last one computed "
                    "(rgb_marched, depth, alphainv_last in image order -- also with --shuffle-rays --, float32) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true", help="also measure and check everything beyond the headline: per-kernel times and "
                    "roofline, CPU baseline and parity, scaling proxy / weak scaling / frame assembly check (N > 1), secondary scenes, "
                    "training steps, detail file")
    return ap.parse_args()


def _rgbnet(g, device, C, pe):
    dims = [C + 3 + 6 * pe, 128, 128, 3]
    ws, bs = [], []
    for i in range(3):
        b = 1.0 / math.sqrt(dims[i])
        ws.append(torch.empty(dims[i + 1], dims[i], device=device).uniform_(-b, b, generator=g))
        bs.append(torch.empty(dims[i + 1], device=device).uniform_(-b, b, generator=g))
    bs[2].zero_()  # nn.init.constant_(rgbnet[-1].bias, 0)  (FourierGrid_model.py:241)
    return ws, bs


def _state(dens, k0, ws, bs, G, F, pe, norm="inf"):
    return {
        "density_grid": dens, "k0_grid": k0, "rgbnet_weights": ws, "rgbnet_biases": bs,
        "scene_center": torch.zeros(3), "scene_radius": torch.ones(3),
        "xyz_min": torch.Tensor([-1, -1, -1]) - 0.2, "xyz_max": torch.Tensor([1, 1, 1]) + 0.2,
        "bg_len": 0.2, "fourier_freq_num": F, "viewbase_pe": pe,
        "act_shift": float(torch.FloatTensor([math.log(1 / (1 - 1e-4) - 1)])), "voxel_size_ratio": 1.0,
        "fast_color_thres": 1e-4, "contracted_norm": norm, "world_len": G,
    }


def make_state(G, device, seed, F=3):
    """S1: synthetic FourierGridModel parameters generated ON the device (no dataset / checkpoint in the image):
    density.grid ~ N(mu, sigma^2), k0.grid ~ N(0,1), rgbnet with nn.Linear's default init."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    C, pe = 12, 4
    P = 1 + 2 * F
    dens = torch.empty(P, 1, G, G, G, device=device).normal_(DENS_MEAN, DENS_STD, generator=g)
    k0 = torch.empty(P, C, G, G, G, device=device).normal_(0.0, 1.0, generator=g)
    ws, bs = _rgbnet(g, device, C, pe)
    return _state(dens, k0, ws, bs, G, F, pe)


def make_state_surfaces(G, device, seed, C=12, pe=4, norm="inf", F=3):
    """S1b (and, with C=3, pe=2, norm='l2', G=300, one S5 Waymo-style block): the model shape with TRAINED-LIKE statistics -- smooth fields, opaque surfaces, empty space below the
    alpha threshold.  Level 0 of the density grid carries 7x a smooth occupancy field (soft spheres, a ground slab and
    the lower half of the contracted far shell; 1.5-voxel transitions between raw density -6 and +16, so empty space
    has alpha ~3e-7 < thres and solids saturate in 1-2 samples); the six sin/cos levels and all k0 levels are low-pass
    noise.  Rays that look down end on a surface (T < 1e-3), rays that look up leave through empty sky."""
    g = torch.Generator(device=device)
    g.manual_seed(seed + 1000)
    P = 1 + 2 * F
    lin = torch.linspace(-1.2, 1.2, G, device=device)
    X, Y, Z = torch.meshgrid(lin, lin, lin, indexing="ij")
    w = 1.5 * 2.4 / (G - 1)                                     # transition half-width: 1.5 voxels
    occ = torch.sigmoid((-0.45 - Z) / w)                        # ground slab z < -0.45
    cheb = torch.maximum(torch.maximum(X.abs(), Y.abs()), Z.abs())
    occ = torch.maximum(occ, torch.sigmoid((cheb - 1.12) / w) * (Z < 0.1).float())    # lower far shell
    cg = torch.Generator()
    cg.manual_seed(seed + 7)
    eye = camera(0, "cpu")[:, 3]
    placed = 0
    while placed < 14:                                          # soft spheres around the scene centre, clear of the camera
        ct = torch.rand(3, generator=cg) * 1.4 - 0.7
        r = float(torch.rand(1, generator=cg) * 0.2 + 0.08)
        if float((ct - eye).norm()) < r + 0.12:
            continue
        placed += 1
        c = ct.tolist()
        dist_c = ((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2).sqrt()
        occ = torch.maximum(occ, torch.sigmoid((r - dist_c) / w))
    del X, Y, Z, cheb
    target = -6.0 + 22.0 * occ                                  # raw density the mean over levels should produce

    def smooth_noise(n_ch, amp):
        x = torch.empty(n_ch, 1, G, G, G, device=device).normal_(0.0, 1.0, generator=g)
        for _ in range(2):                                      # two 5^3 box filters ~ a smooth field
            x = torch.nn.functional.avg_pool3d(x, 5, stride=1, padding=2, count_include_pad=False)
        return x / x.std() * amp

    dens = smooth_noise(P, 2.0).reshape(P, 1, G, G, G)
    dens[0, 0] = P * target                                     # the mean over the P levels restores `target` (+- noise)
    k0 = torch.empty(P, C, G, G, G, device=device)
    for l in range(P):
        k0[l] = smooth_noise(C, 1.0)[:, 0]
    ws, bs = _rgbnet(g, device, C, pe)
    return _state(dens.contiguous(), k0, ws, bs, G, F, pe, norm)


def camera(rank, device):
    """Look-at-origin pinhole camera; `rank` picks an azimuth (weak-scaled frames differ per rank)."""
    ang = 0.35 * rank
    eye = torch.tensor([0.3 * math.cos(ang) - 0.2 * math.sin(ang), 0.3 * math.sin(ang) + 0.2 * math.cos(ang), 0.4])
    fwd = -eye / eye.norm()
    up = torch.tensor([0.0, 0.0, 1.0])
    right = torch.linalg.cross(fwd, up)
    right = right / right.norm()
    up2 = torch.linalg.cross(right, fwd)
    c2w = torch.stack([right, up2, -fwd, eye], dim=1)  # OpenGL-style: camera looks along -z
    return c2w.to(device)


def lib_sha16():
    from unboundednerfpytorch_amd import _lib
    return hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]


def elf_section(path, name, with_offset=False):
    """bytes of one section of an ELF64 file (no external tools needed); with_offset: (file offset, bytes)"""
    import struct
    b = open(path, "rb").read()
    assert b[:4] == b"\x7fELF" and b[4] == 2, "not an ELF64 file"
    shoff, = struct.unpack_from("<Q", b, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)
    sec = lambda i: struct.unpack_from("<IIQQQQIIQQ", b, shoff + i * shentsize)
    stroff, strsize = sec(shstrndx)[4], sec(shstrndx)[5]
    strtab = b[stroff: stroff + strsize]
    for i in range(shnum):
        h = sec(i)
        nm = strtab[h[0]: strtab.index(b"\0", h[0])].decode()
        if nm == name:
            return (h[4], b[h[4]: h[4] + h[5]]) if with_offset else b[h[4]: h[4] + h[5]]
    return None


def device_code_sha16(path=None):
    """sha256 of the library's .hip_fatbin section = the gfx950 code objects themselves.  The whole-file hash also covers
    .comment / .symtab / .strtab, which differ between two builds of identical device code (the driver's
    box and the profiling box disagreed on the file hash, not on the code); static PMC counters are keyed on THIS."""
    from unboundednerfpytorch_amd import _lib
    sec = elf_section(path or _lib.LIB_PATH, ".hip_fatbin")
    return hashlib.sha256(sec).hexdigest()[:16] if sec is not None else None


class FrameBench:
    """One scene on this rank: renderer + camera + the timed step (ray generation, shard, render, tile exchange)."""

    def __init__(self, args, state, device, world, rank, dist, renderer=None):
        """renderer: test hook (tests/test_host_logic.py drives the sharding / exchange logic over gloo with a stand-in
        that has the renderer's call signature); None = the HIP FourierGridRenderer."""
        from unboundednerfpytorch_amd.dist import shard_bounds, tile_assignment
        from unboundednerfpytorch_amd.fourier_render import get_rays_of_a_view, get_rays_of_pixel_index, pixel_tile_order
        self.get_rays, self.get_rays_idx = get_rays_of_a_view, get_rays_of_pixel_index
        self.args, self.device, self.world, self.rank, self.dist = args, device, world, rank, dist
        H, W, G = args.height, args.width, args.grid
        self.H, self.W = H, W
        self.stepsize = 1.31 * G / 200.0 if G != 200 else 1.31
        if getattr(args, "stepsize", None):
            self.stepsize = float(args.stepsize)      # e.g. 0.5: garden_single.py's own sampling (S = 668 at G = 200)
        if renderer is None:
            from unboundednerfpytorch_amd.fourier_render import FourierGridRenderer
            renderer = FourierGridRenderer(state, device, pipeline=args.pipeline, mlp_mode=args.mlp_mode)
        self.rend = renderer
        # the frame's rays are in pixel-block (or row-segment) order by construction: no coherence check (= no host sync) in
        # the timed step; --shuffle-rays measures the raw kernels on incoherent tiles, so it opts out of the renderer's sort too
        self.rkw = {"ray_order": "coherent"} if renderer.__class__.__name__ == "FourierGridRenderer" else {}
        self.K = [[1600.0 * W / 1920.0, 0, W / 2.0], [0, 1600.0 * W / 1920.0, H / 2.0], [0, 0, 1]]
        self.R = H * W
        self.S = self.rend.tables(self.stepsize)[2]
        self.c2w = camera(0, device)
        self.use_dist = dist is not None
        # the deal (see --deal): contiguous bands unless tiles are dealt singly, by block rows of the image, or in groups of K
        dg = int(getattr(args, "deal_group", 0) or 0)
        deal = getattr(args, "deal", "bands")
        self.deal_group = dg if dg > 0 else (max(1, W // 8) if deal == "rows" else 1)
        self.contiguous = bool(getattr(args, "contiguous", False)) or (dg <= 0 and deal == "bands")
        if world > 1 and not self.contiguous:
            self.idx = tile_assignment(self.R, world, rank, group=self.deal_group).to(device)
            self.per = tile_assignment(self.R, world, 0, group=self.deal_group).numel()
            self.bounds = None
        else:
            self.idx = None
            self.bounds = shard_bounds(self.R, world, rank)
            self.per = shard_bounds(self.R, world, 0)[1]
        # the frame's ray order: 8 x 8 pixel blocks (one per march wave) unless --ray-tile 0 / --shuffle-rays / odd sizes
        T = getattr(args, "ray_tile", 0)
        self.order = None
        if T > 1 and not getattr(args, "shuffle_rays", False):
            self.order = pixel_tile_order(H, W, device, T)
        self.tile = T
        # this rank's flat pixel indices (constant over the frames): only its own rays are generated per step
        if self.idx is not None:
            self.px = self.idx.to(torch.int64).contiguous()
        else:
            b, e = self.bounds
            self.px = torch.arange(b, e, dtype=torch.int64, device=device)
        if self.order is not None:
            self.px = self.order[self.px].contiguous()
        self.gathered = [torch.empty(world * self.per, 5, device=device) for _ in range(2)] if self.use_dist else None
        self.inflight = {"work": None, "n": 0, "tile": None}
        self.assembled_ev = [None, None]      # gathered[i] may be overwritten by the next exchange only after its frame has been assembled
        fp = int(getattr(args, "frame_pair", -1))
        self.pair = None
        if fp != 0 and device.type == "cuda" and hasattr(self.rend, "use_workspace_slot"):      # (default: on; --frame-pair 0 = one stream)
            self.pair = [torch.cuda.Stream(device) for _ in range(max(2, int(getattr(args, "frames_in_flight", 3))))]      # frames take them in turn (step)
            # every stream's work list is resident before anything is timed (an 8.4 GiB allocation is set-up, not a step): the frame's
            # size at N = 1 and for a rank's own whole frames, a rank's share of it when ranks share one GPU (debugging runs)
            n_rays = self.per if (world > 1 and os.environ.get("UGRID_BENCH_SHARE_GPU") == "1") else self.R
            for k in range(len(self.pair)):
                self.rend.use_workspace_slot(k)
                self.rend._workspace(min(n_rays, self.rend.rays_per_chunk(self.S)), self.S)
            self.rend.use_workspace_slot(0)
            # ... and every stream has its hardware queue (created on a stream's first use, ~10 ms): with fewer warm-up steps than streams
            # that first use would fall inside the timed region (steps 10 / warmup 2: 9.8 instead of 8.2 ms per frame)
            for st in self.pair:
                with torch.cuda.stream(st):
                    torch.zeros(1, device=device)
            torch.cuda.synchronize(device)
        self.single_stream = False      # timed(single_stream=True): the pair switched off for one timed region
        self.n_step = 0
        self.last_out = None
        self.frame = None
        # row of the gathered [world*per,5] buffer that holds image pixel i: undoes the tile dealing (or the bands) and the
        # 8 x 8 pixel-block ray order in ONE index_select per frame, inside the timed step
        self.src_index = None
        if self.use_dist:
            pix_of_row = torch.full((world * self.per,), -1, dtype=torch.int64)
            for r in range(world):
                if self.idx is not None:
                    ir = tile_assignment(self.R, world, r, group=self.deal_group)
                else:
                    b, e = shard_bounds(self.R, world, r)
                    ir = torch.arange(b, e, dtype=torch.int64)
                pix_of_row[r * self.per: r * self.per + ir.numel()] = ir if self.order is None else self.order.cpu()[ir]
            rows = torch.nonzero(pix_of_row >= 0).reshape(-1)
            src = torch.empty(self.R, dtype=torch.int64)
            src[pix_of_row[rows]] = rows
            self.src_index = src.to(device)

    def rays(self, c2w=None):
        ro, rd, vd = self.get_rays(self.H, self.W, self.K, self.c2w if c2w is None else c2w)
        ro, rd, vd = ro.reshape(-1, 3), rd.reshape(-1, 3), vd.reshape(-1, 3)
        if getattr(self.args, "shuffle_rays", False):
            if not hasattr(self, "_perm"):
                g = torch.Generator(device=self.device)
                g.manual_seed(1234)
                self._perm = torch.randperm(ro.shape[0], device=self.device, generator=g)
            ro, rd, vd = ro[self._perm], rd[self._perm], vd[self._perm]
        return ro, rd, vd

    def my_shard(self, ro, rd, vd):
        if self.idx is not None:
            return ro[self.idx].contiguous(), rd[self.idx].contiguous(), vd[self.idx].contiguous()
        b, e = self.bounds
        return ro[b:e].contiguous(), rd[b:e].contiguous(), vd[b:e].contiguous()

    def step(self, timing=None, weak=False):
        """strong (default): this rank's shard of THE frame; weak: a whole frame of its own camera.  With a stream pair (--frame-pair) the
        whole step -- ray generation, march, shade, exchange -- is issued on stream k & 1 with work list k & 1: two frames are in flight,
        nothing of frame k + 1 waits for frame k except the exchange's own hand-over (the frames of a view list are independent)."""
        if self.pair is None or self.single_stream or (weak and os.environ.get("UGRID_BENCH_SHARE_GPU") == "1"):
            # (ranks SHARING one GPU -- debugging runs -- keep one work list for their whole weak-scaled frame: N x 2 x 8.4 GB do not fit)
            if self.pair is not None:
                self.rend.use_workspace_slot(0)
            return self._step(timing, weak)
        k = self.n_step % len(self.pair)
        self.n_step += 1
        if self.n_step <= len(self.pair):
            self.pair[k].wait_stream(torch.cuda.current_stream(self.device))      # (what set up the inputs ran on the caller's stream)
        self.rend.use_workspace_slot(k)
        with torch.cuda.stream(self.pair[k]):
            return self._step(timing, weak)

    def _step(self, timing=None, weak=False):
        # ray generation is inside the step: the whole frame (weak / 1 GPU) or this rank's pixels of it (strong)
        if self.order is not None and (weak or self.world == 1):
            ro, rd, vd = self.get_rays_idx(self.H, self.W, self.K, camera(self.rank, self.device) if weak else self.c2w, self.order)
        elif not weak and self.world > 1:
            ro, rd, vd = self.get_rays_idx(self.H, self.W, self.K, self.c2w, self.px)
        else:
            ro, rd, vd = [x.contiguous() for x in self.rays(camera(self.rank, self.device) if weak else None)]
        out = self.rend(ro, rd, vd, stepsize=self.stepsize, render_depth=True, timing=timing, **self.rkw)
        if self.order is not None and (weak or self.world == 1):       # back to image order (inside the timed step)
            from unboundednerfpytorch_amd.fourier_render import untile
            out = dict(out, **{k: untile(out[k], self.H, self.W, self.tile) for k in ("rgb_marched", "depth", "alphainv_last") if k in out})
        self.last_out = out
        if self.use_dist and not weak:
            # the one exchange step of the path: rendered tiles [R/N,5] = rgb(3), depth, alphainv_last -> every rank
            n = out["depth"].shape[0]
            tile = torch.zeros(self.per, 5, device=self.device) if n < self.per else torch.empty(self.per, 5, device=self.device)
            tile[:n, 0:3] = out["rgb_marched"]
            tile[:n, 3] = out["depth"]
            tile[:n, 4] = out["alphainv_last"]
            fl = self.inflight
            if fl["work"] is not None:
                fl["work"].wait()                # stream-level wait for the previous frame's exchange
                self._assemble()                 # ... whose image is put together while this frame's exchange runs
            ev = self.assembled_ev[fl["n"] & 1]
            if ev is not None:               # (with frames on two streams the assembly of frame k - 2 ran on the OTHER stream)
                torch.cuda.current_stream(self.device).wait_event(ev)
            fl["work"] = self.dist.all_gather_into_tensor(self.gathered[fl["n"] & 1], tile, async_op=True)
            fl["tile"] = tile                    # keep the send buffer alive until the collective has run
            fl["n"] += 1
        return out

    def _assemble(self):
        """gathered tiles -> the frame in image order [R,5] (un-deal + un-tile: one index_select), part of the step"""
        full = self.gathered[(self.inflight["n"] - 1) & 1]
        self.frame = torch.index_select(full, 0, self.src_index)
        if self.device.type == "cuda":
            self.assembled_ev[(self.inflight["n"] - 1) & 1] = torch.cuda.current_stream(self.device).record_event()

    def barrier(self):
        if self.use_dist:
            if self.inflight["work"] is not None:
                self.inflight["work"].wait()     # the last exchange and its assembly are inside the timed region
                self.inflight["work"] = None
                self._assemble()
            self.dist.barrier()
        if self.device.type == "cuda":
            torch.cuda.synchronize()

    def assembled_frame(self):
        """The last exchanged frame in image order, [R,5] = rgb(3), depth, alphainv_last (every rank holds it): assembled
        inside the timed step by _assemble()."""
        return self.frame

    def timed(self, steps, warmup, weak=False, single_stream=False):
        """K steps between two barriers.  single_stream: the same K steps issued on ONE stream with ONE work list (each kernel has the
        chip to itself: what the per-kernel HIP-event durations and the roofline are quoted on when the frames of the headline region
        overlap on the stream pair)."""
        self.barrier()
        self.single_stream = bool(single_stream)
        try:
            return self._timed(steps, warmup, weak)
        finally:
            self.single_stream = False

    def _timed(self, steps, warmup, weak):
        for _ in range(warmup):
            self.step(weak=weak)
        self.barrier()
        timing = []
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step(timing, weak=weak)
        self.barrier()
        dt = time.perf_counter() - t0
        if self.use_dist:
            t = torch.tensor([dt], device=self.device, dtype=torch.float64)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt, timing

    def check_exchange(self):
        """this rank's tile must sit at its slot of the gathered frame"""
        if not self.use_dist:
            return
        out = self.last_out
        n = out["depth"].shape[0]
        mine = self.gathered[(self.inflight["n"] - 1) & 1][self.rank * self.per: self.rank * self.per + n]
        assert torch.equal(mine[:, 0:3], out["rgb_marched"]) and torch.equal(mine[:, 4], out["alphainv_last"])

    def full_frame(self):
        """The whole frame rendered on this rank (for survivor statistics and parity): untimed."""
        ro, rd, vd = [x.contiguous() for x in self.rays()]
        self.rend.pipeline = 0
        M = 0
        outs = []
        chunk = self.rend.rays_per_chunk(self.S)
        for b in range(0, self.R, chunk):
            e = min(self.R, b + chunk)
            outs.append(self.rend(ro[b:e], rd[b:e], vd[b:e], stepsize=self.stepsize, render_depth=True, **self.rkw))
            M += self.rend.survivors_of_last_chunk()
        out = {k: torch.cat([o[k] for o in outs]) for k in ("rgb_marched", "depth", "alphainv_last")}
        return (ro, rd, vd), out, M


def timed_with_kernels(fb, steps, warmup):
    """(seconds of the K-step region, per-kernel ms, seconds of the one-stream region or None): the throughput region as configured
    (two frames in flight by default) and, when that overlaps launches, a second region of the same K steps on one stream for the
    per-kernel HIP-event durations."""
    dt, timing = fb.timed(steps, warmup)
    dt1 = None
    if fb.pair is not None:
        dt1, timing = fb.timed(steps, 1, single_stream=True)
    return dt, kernel_ms(timing, steps), dt1


def kernel_ms(timing, steps):
    # (pipelined frames carry 4 events per chunk; the kernels of neighbouring chunks overlap then)
    return {"render_march": sum(ev[0].elapsed_time(ev[1]) for ev, _ in timing) / steps,
            "render_shade": sum(ev[-2].elapsed_time(ev[-1]) for ev, _ in timing) / steps}


DUMP_BUDGET = 64 * 10 ** 6 - 4096      # bytes of .npy files --dump-outputs may write (64 MB, less room for the headers)


def dump_outputs(fb, out_dir):
    """--dump-outputs: the frame the LAST timed step computed, as a caller of the step receives it -- per-ray rgb_marched [R,3], depth [R],
    alphainv_last [R] in image order (N > 1: the frame assembled from every rank's tiles; --shuffle-rays: put back from the shuffled
    order) -- as out_dir/<name>.npy, float32.  A frame larger than DUMP_BUDGET is written as a fixed, seeded sample of its rays (the
    same rows of every array).  Returns the file names."""
    import numpy as np
    keys = ("rgb_marched", "depth", "alphainv_last")
    if fb.use_dist:
        f = fb.assembled_frame()
        outs = {"rgb_marched": f[:, 0:3], "depth": f[:, 3], "alphainv_last": f[:, 4]}
    else:
        outs = {k: fb.last_out[k] for k in keys}
    outs = {k: outs[k].detach().to("cpu", torch.float32).contiguous() for k in keys}
    perm = getattr(fb, "_perm", None)
    if perm is not None:        # --shuffle-rays on one rank: the timed steps rendered the shuffled list, row i = pixel perm[i]
        perm = perm.cpu()
        outs = {k: torch.empty_like(v).index_copy_(0, perm, v) for k, v in outs.items()}
    R = outs["depth"].shape[0]
    per_ray = sum(v.numel() // max(1, R) for v in outs.values()) * 4
    if R * per_ray > DUMP_BUDGET:
        g = torch.Generator()
        g.manual_seed(0)
        idx = torch.randperm(R, generator=g)[:DUMP_BUDGET // per_ray].sort().values
        outs = {k: v[idx] for k, v in outs.items()}
    os.makedirs(out_dir, exist_ok=True)
    for k, v in outs.items():
        np.save(os.path.join(out_dir, k + ".npy"), v.numpy())
    return [k + ".npy" for k in keys]


def _profile_path(name, code=None):
    """profiles/<this round>/<name>; if it is absent (or holds counters of another device code) and an earlier round's file of
    that name was taken on `code`, that one -- static counters stay valid exactly as long as the kernels' binary does"""
    first = os.path.join(PROFILE_DIR, name)
    cands = [first] + [os.path.join(os.path.dirname(PROFILE_DIR), r, name) for r in PROFILE_FALLBACK]
    for c in cands:
        j = _load_json(c)
        if j is not None and (code is None or j.get("device_code_sha16") == code):
            return c
    return first


def _load_json(path):
    try:
        return json.load(open(path))
    except Exception:
        return None


def roofline_block(kern, M, R, S, shade_passes, frame_rays=None, P=7, ms_per_step=None, pmc_workload_ok=True):
    """Per-kernel utilisation of every candidate limit, and ONE summary entry: always the frame kernel with the LOWER fraction of
    its roof (no window, no tie rule: VERDICT r3 weak #4).

    What the roof is.  SURVEY 8d's algorithmic gather bytes (224 B per sample, 2688 B per survivor) are served by the caches:
    divided by the HBM peak they give > 1 (`frac_of_hbm_algorithmic`, printed in the summary entry itself so that it cannot be
    misread as a roofline fraction).  The unit they all pass is the per-CU vector-memory address / data path (TA + TCP): one
    64-byte quad per clock per CU, i.e. 16 clocks per 1-KiB `global_load_dwordx4` wave instruction, 39.3 TB/s for the chip at
    2.4 GHz.  That peak is not in MI355X_MICROARCH.md; it stands on two measurements committed under profiles/: the micro-benchmark
    (63.8 / 61.6 B/clk/CU, profiles/r03/microbench_l1_dwordx4.json) and, since round 4, the hardware's own counters on these
    kernels (profiles/r04/pmc_summary.json): TA_TA_BUSY per TA_FLAT_READ_WAVEFRONTS = 18.9 (march) / 21 (shade) clocks per wave
    instruction against the 16 of the peak, and `ta_busy_measured` = the fraction of the launch during which the CU's TA was
    busy (0.92 march, 0.73 shade) -- THE counter-backed utilisation of the binding unit.  `frac` = achieved / peak at the nominal
    clock; `ta_busy_measured` is at the clock the launch really had (the chip runs these kernels at its power limit, ~2.0 GHz).

    HBM: `traffic` = memory-side bytes from the request counters (TCC_EA0_RDREQ_{32B,64B,128B}; = 2 x FETCH_SIZE for every access
    shape on gfx950, calibrated by tools/microbench/fetch_calib.hip: the L2 issues 128-byte requests that FETCH_SIZE tallies at
    64 B) + WRITE_SIZE.  VALU: instruction counts x 2 clocks per SIMD.  Matrix pipe: SQ_VALU_MFMA_BUSY_CYCLES.
    Static counters are merged ONLY when taken on the same device code (`device_code_sha16` = sha256 of .hip_fatbin); times are
    live HIP events of this run."""
    code = device_code_sha16()
    ppath = _profile_path("pmc_summary.json", code)
    pmc = _load_json(ppath) or {}
    pmc_refused = None
    if pmc and pmc.get("device_code_sha16") != code:
        pmc_refused = "counters of %s were taken on device code %s, this library is %s" % (
            os.path.relpath(ppath, ROOT), pmc.get("device_code_sha16"), code)
        pmc = {}
    elif pmc and not pmc_workload_ok:
        pmc_refused = "counters of %s were taken on the default S1 frame, this run renders another workload" % os.path.relpath(ppath, ROOT)
        pmc = {}
    scale = 1.0 if not frame_rays else R / float(frame_rays)     # counters are per whole-frame launch: a rank's share
    l1m = (_load_json(os.path.join(PROFILE_DIR, "microbench_l1_dwordx4.json"))
           or _load_json(os.path.join(ROOT, "profiles", "r03", "microbench_l1_dwordx4.json")) or {})     # (measured in round 3)
    l1_meas_bpc = l1m.get("quad64_B_per_clk_per_CU")             # the shade gather's access shape: 64 B per lane quad
    l1_meas_lin = l1m.get("linear_B_per_clk_per_CU")
    alg = {"render_march": R * S * 32 * P + R * 32,  # 8 coefficients x P levels x 4 B per sample (224 B at P = 7) + rays in / (depth, alphainv) out
           "render_shade": M * 384 * P + R * 24}     # x 12 channels per survivor (2688 B at P = 7) + viewdirs in / rgb out
    # executed f16 MFMA flops of the fp16x2 rgbnet: 132 MFMAs (32x32x16) per 32-survivor pass; USEFUL rgbnet flops:
    # 2 x (39 x 128 + 128 x 128 + 128 x 3) = 43 520 per survivor
    mfma_flops = {"render_march": 0.0, "render_shade": shade_passes * 132 * 32 * 32 * 16 * 2.0}
    useful_flops = {"render_march": 0.0, "render_shade": M * 43520.0}
    per = {}
    for name, ms in kern.items():
        if name not in alg:
            continue
        t = ms * 1e-3
        c = pmc.get(name, {})
        e = {"ms": ms, "algorithmic_bytes": alg[name], "algorithmic_GBps": alg[name] / t / 1e9,
             "frac_of_hbm_algorithmic": alg[name] / t / 1e9 / HBM_PEAK_GBS,
             "frac_of_hbm_algorithmic_note": "> 1 = cache-served: SURVEY 8d's logical gather bytes never reach HBM, NOT a roofline fraction",
             "l1_frac": alg[name] / t / 1e9 / L1_PEAK_GBS,
             "mfma_TFLOPs": mfma_flops[name] / t / 1e12, "mfma_frac": mfma_flops[name] / t / 1e12 / MFMA_F16_PEAK_TFLOPS,
             "mfma_useful_TFLOPs": useful_flops[name] / t / 1e12}
        if l1_meas_bpc:
            e["l1_frac_of_measured_peak"] = alg[name] / t / (N_CU * l1_meas_bpc * CLK_HZ)
        if "hbm_bytes" in c:
            e["hbm_bytes_pmc"] = c["hbm_bytes"] * scale
            e["hbm_GBps"] = e["hbm_bytes_pmc"] / t / 1e9
            e["hbm_frac"] = e["hbm_GBps"] / HBM_PEAK_GBS
            e["algorithmic_over_hbm_bytes"] = alg[name] / max(1.0, e["hbm_bytes_pmc"])
        if "valu_insts" in c:
            e["valu_Ginst_per_s"] = c["valu_insts"] * scale / t / 1e9
            e["valu_frac"] = e["valu_Ginst_per_s"] / VALU_PEAK_GINST
        # counter-backed vector-L1 evidence (round 4): tag look-ups, hit rate, TA busy, clocks per wave instruction
        for k_src, k_dst in (("l1_accesses", "l1_tag_lookups_64B"), ("l1_hit_rate", "l1_hit_rate_measured"), ("ta_busy_frac", "ta_busy_measured"),
                             ("ta_clocks_per_wave_instruction", "ta_clocks_per_wave_instruction"), ("lds_array_busy_frac", "lds_array_busy_measured"),
                             ("l2_hit_rate", "l2_hit_rate_measured")):
            if k_src in c:
                e[k_dst] = c[k_src] * (scale if k_src == "l1_accesses" else 1.0)
        for k_src in ("sq_wait_any_of_wave_cycles", "sq_wait_inst_any_of_wave_cycles", "sq_active_inst_any_of_wave_cycles"):
            if k_src in c:
                e[k_src] = c[k_src]
        if "rocprofv3_avg_ms" in c:
            # the average duration of this kernel in the committed `rocprofv3 --kernel-trace --stats` run of the same command
            # (profiles/r05/bench_s1_kernel_stats.csv): the live HIP-event time above must agree with it
            e["rocprofv3_avg_ms"] = c["rocprofv3_avg_ms"] * scale
            e["hip_event_over_rocprofv3"] = ms / max(1e-9, c["rocprofv3_avg_ms"] * scale)
        if "gui_active_cycles" in c and scale == 1.0:
            # the chip runs these kernels at its power-limited clock, well below the 2.4 GHz the peaks assume: the same
            # counts against the cycles the kernel actually had (profiled launch) = how busy the units were
            cyc = c["gui_active_cycles"]
            e["effective_clock_GHz_profiled"] = cyc / (c.get("pmc_pass_avg_ms", c.get("rocprofv3_avg_ms", ms)) * 1e-3) / 1e9
            if "valu_insts" in c:
                e["valu_issue_busy"] = c["valu_insts"] * 2.0 / N_SIMD / cyc
            if "mfma_busy_cycles" in c:
                e["mfma_pipe_busy"] = c["mfma_busy_cycles"] / N_SIMD / cyc
            e["l1_path_busy"] = alg[name] / (N_CU * 64.0) / cyc
            if l1_meas_bpc:
                e["l1_path_busy_vs_measured_peak"] = alg[name] / (N_CU * float(l1_meas_bpc)) / cyc
        fr = {k[:-5]: v for k, v in e.items() if k.endswith("_frac")}
        e["bound"] = max(fr, key=fr.get)
        per[name] = e
    if not per:
        return None
    # ALWAYS the kernel further from its roof (the lower of the kernels' best fractions): the conservative entry
    dom = min(per, key=lambda k: max(v for kk, v in per[k].items() if kk.endswith("_frac")))
    d = per[dom]
    units = {"hbm": ("GB/s", d.get("hbm_GBps"), HBM_PEAK_GBS), "l1": ("GB/s", d["algorithmic_GBps"], L1_PEAK_GBS),
             "mfma": ("TFLOP/s", d["mfma_TFLOPs"], MFMA_F16_PEAK_TFLOPS),
             "valu": ("Ginst/s", d.get("valu_Ginst_per_s"), VALU_PEAK_GINST)}
    unit, ach, peak = units[d["bound"]]
    frame_hbm = sum(p.get("hbm_bytes_pmc", 0) for p in per.values())
    frame_ms = sum(p["ms"] for p in per.values())
    src = os.path.relpath(ppath, ROOT) if pmc else None
    return {"kernel": dom, "kernel_choice": "the frame kernel with the LOWER fraction of its roof (always; both are in per_kernel)",
            "bound": d["bound"], "bound_note": "l1 = the per-CU vector-memory path (TA/TCP, 64 B per clock per CU): see bench.roofline_block",
            "achieved": ach, "peak": peak, "unit": unit, "frac": ach / peak,
            "ta_busy_measured": d.get("ta_busy_measured"),
            "traffic": d.get("hbm_bytes_pmc"), "hbm_frac_measured": d.get("hbm_frac"),
            "frac_of_hbm_algorithmic": d["frac_of_hbm_algorithmic"],
            "frac_of_hbm_algorithmic_note": "algorithmic bytes / time / 8 TB/s: > 1 because the gather bytes are cache-served -- "
                                            "NOT a roofline fraction; the HBM fraction of this kernel is hbm_frac_measured",
            "peaks": {"hbm_GBps": HBM_PEAK_GBS, "l1_GBps_nominal_64B_per_clk_per_CU": L1_PEAK_GBS,
                      "l1_B_per_clk_per_CU_measured": {"quad_64B_gather": l1_meas_bpc, "linear_1KiB_per_wave": l1_meas_lin,
                                                       "source": "profiles/r03/microbench_l1_dwordx4.json" if l1m else None},
                      "mfma_f16_TFLOPs": MFMA_F16_PEAK_TFLOPS,
                      "valu_Ginst_per_s": VALU_PEAK_GINST, "clock_GHz_assumed": CLK_HZ / 1e9},
            "frame": frame_block(per, alg, mfma_flops, useful_flops, frame_ms, frame_hbm, ms_per_step, P),
            "pmc_source": src, "pmc_device_code_sha16": pmc.get("device_code_sha16"),
            "pmc_refused": pmc_refused, "pmc_scaled_to_rank_share": scale if scale != 1.0 else None,
            "per_kernel": per}


def frame_block(per, alg, mfma_flops, useful_flops, kernels_ms, frame_hbm, ms_per_step, P):
    """The whole frame against the two peaks MI355X_MICROARCH.md lists: every number one line of arithmetic from
    the committed profiles (profiles/r05/pmc_summary.json, bench_s1_kernel_stats.csv) + the guide.  `ms` = the step time the line's
    `value` is computed from (ray generation + march + shade + un-tiling) when given, else the two kernels' sum."""
    ms = ms_per_step if ms_per_step else kernels_ms
    t = ms * 1e-3
    alg_total = sum(alg.values())
    shade = per.get("render_shade", {})
    out = {"ms": ms, "kernels_ms": kernels_ms,
           "algorithmic_bytes": alg_total,
           "algorithmic_bytes_formula": "R*S*32*P + M*384*P + R*56 with P = %d (SURVEY 8d: 224 B per sample, 2688 B per survivor at P = 7)" % P,
           "frac_of_hbm_algorithmic": alg_total / t / 1e9 / HBM_PEAK_GBS,
           "frac_of_hbm_algorithmic_note": "algorithmic gather bytes / step time / 8 TB/s: > 1 because the caches serve them (L1 hit rate 0.93) -- "
                                           "NOT a roofline fraction; the north star's '>= 70 % of the HBM roofline' cannot describe a cache-blocked gather",
           "hbm_bytes_pmc": frame_hbm or None,
           "hbm_frac": (frame_hbm / t / 1e9 / HBM_PEAK_GBS) if frame_hbm else None,
           "hbm_frac_note": "counter HBM bytes (TCC_EA0 request sizes + WRITE_SIZE) of march + shade / step time / 8 TB/s",
           "mfma_executed_TFLOPs": sum(mfma_flops.values()) / t / 1e12,
           "mfma_executed_frac_of_2.5PF": sum(mfma_flops.values()) / t / 1e12 / MFMA_F16_PEAK_TFLOPS,
           "mfma_useful_TFLOPs": sum(useful_flops.values()) / t / 1e12,
           "mfma_useful_frac_of_2.5PF": sum(useful_flops.values()) / t / 1e12 / MFMA_F16_PEAK_TFLOPS,
           "mfma_note": "executed = 132 v_mfma_f32_32x32x16_f16 per 32-survivor pass (fp16x2: three products per useful one, K padded 39 -> 48); "
                        "useful = 43 520 flop per survivor (SURVEY 8d); over the WHOLE step time -- over the shade kernel alone: "
                        "%.3f executed / %.3f useful of 2.5 PFLOP/s" % (shade.get("mfma_frac", 0.0), shade.get("mfma_useful_TFLOPs", 0.0) / MFMA_F16_PEAK_TFLOPS),
           "clock_GHz_profiled": {k: v.get("effective_clock_GHz_profiled") for k, v in per.items()},
           "clock_note": "GRBM_GUI_ACTIVE / 8 XCDs / the launch's duration in the counter pass; the peaks above assume 2.4 GHz"}
    return out


def hbm_roofline_entry(r):
    """The one kernel of the path the north star's "fraction of the HBM roofline" can be checked on: the fused
    dense TV + Adam pass over S3's k0 grid streams seven 3.46 GB arrays, each byte once.  `achieved` = algorithmic bytes / the live
    HIP-event time; `traffic` = the bytes the launch really moved (TCC_EA0 read / write request counters of a separate rocprofv3 --pmc
    pass, profiles/r05/tv_adam_dense_pmc.json, merged only for the same device code)."""
    out = {"kernel": r["kernel"], "bound": "hbm", "achieved": r["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": r["achieved"] / HBM_PEAK_GBS,
           "ms": r["ms"], "algorithmic_bytes": r["algorithmic_bytes"], "traffic": None,
           "note": "ugrid_tv_adam_dense_cl on the S3 k0 grid (P = 9, C = 12, 200^3, channel-last): 7 arrays x 3.456e9 B, each byte once; "
                   "frac = algorithmic bytes / time / 8 TB/s (the guide's spec peak; ~6.3 TB/s is what it calls achievable: %.2f of that)"
                   % (r["achieved"] / 6300.0)}
    tpath = _profile_path("tv_adam_dense_pmc.json", device_code_sha16())
    p = _load_json(tpath)
    if p and p.get("device_code_sha16") == device_code_sha16():
        out["traffic"] = p.get("hbm_bytes")
        out["traffic_read_bytes"], out["traffic_write_bytes"] = p.get("hbm_read_bytes"), p.get("hbm_write_bytes")
        out["traffic_over_algorithmic"] = p.get("hbm_bytes") / float(r["algorithmic_bytes"]) if p.get("hbm_bytes") else None
        out["traffic_GBps"] = p.get("hbm_bytes") / (r["ms"] * 1e-3) / 1e9 if p.get("hbm_bytes") else None
        out["pmc_source"] = os.path.relpath(tpath, ROOT)
    elif p:
        out["pmc_refused"] = "counters were taken on device code %s" % p.get("device_code_sha16")
    return out


def s3_train_step_block(device):
    """BASELINE.json configs[2] (S3: truck_single-shaped training step, P = 9, G = 200, 4096 random rays x S = 668) under the
    driver's clock: tools/bench_train_step.run for the dense-TV phase (global_step < tv_dense_before) and the masked-TV
    phase that follows.  Secondary: a failure here never costs the headline line."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_train_step as bts
        out = {}
        for phase, first in (("dense_tv", 1), ("masked_tv", 10001)):
            r = bts.run(bts.parse(["--steps", "24", "--blocks", "3", "--warmup", "4", "--first-step", str(first)]))
            out[phase] = {k: r[k] for k in ("ms_per_step", "phases_ms", "survivors_M", "samples", "rays_per_sec", "tv_phase", "loss", "psnr")}
            out["workload"] = r["workload"]
            if phase == "dense_tv" and r.get("roofline_tv_adam_dense"):
                # the path's one genuinely HBM-bound kernel, priced against the guide's 8 TB/s
                out["roofline_tv_adam_dense"] = r["roofline_tv_adam_dense"]
            torch.cuda.empty_cache()
        # round 6: the same masked-TV step with NO host read in the loop -- the sync-free native step (counts stay on the device) and the
        # loss handed back as a tensor (train_iteration(return_tensors=True): a caller that logs every N steps)
        r = bts.run(bts.parse(["--steps", "24", "--blocks", "3", "--warmup", "4", "--first-step", "10001", "--sync-free", "1", "--lazy-loss", "1"]))
        out["masked_tv_sync_free"] = {k: r[k] for k in ("ms_per_step", "survivors_M", "rays_per_sec", "tv_phase")}
        torch.cuda.empty_cache()
        return out
    except Exception as e:          # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, e)}


def scaling_proxy(args, rend, device, t1_ms, steps=6, t1_pair_ms=None):
    """What a 1-GPU box can say about N > 1: rank r's share of an N-way deal of THE frame rendered ALONE on this
    device -- same kernels, same rays, same bricks as rank r of an N-GPU run (the tile exchange, 5.2 MB per rank at N = 8, is the only
    thing missing) -- for every rank of N = 2, 4, 8 and three deals: single 64-ray tiles round-robin, block ROWS of the image
    round-robin (W / 8 tiles), contiguous bands (the default of --gpus N).  A share's time is the GPU time of its step (ray generation
    + march + shade) between two HIP events, median over `steps` back-to-back steps -- what a rank of a continuously fed N-GPU run
    spends per frame.  (The host clock around single synchronised steps is NOT used: an idle -> busy transition of the queue
    occasionally starts the first kernel 25-80 ms late on these boxes, profiles/r05/share_stall_diag.txt; back-to-back frames do
    not idle.)  The slowest share is the frame time an N-GPU run cannot beat; t(1 GPU) / (N x slowest share) is the efficiency it
    predicts.  Per-share HBM bytes come from a PMC pass (tools/gpu_rank_share.sh -> profiles/r05/rank_share_pmc.jsonl)."""
    try:
        t1p = t1_pair_ms or t1_ms        # (a frame-pair share is compared with the frame-pair whole frame, a one-stream share with the one-stream frame)
        out = {"t1_ms": t1_ms, "t1_frame_pair_ms": t1_pair_ms, "note": "share r of an N-way deal rendered alone on this GPU (no exchange); GPU time per step between HIP events, "
                                       "median of %d back-to-back steps; predicted_efficiency = t1 / (N * slowest share)" % steps}
        W = args.width
        deals = (("tiles_round_robin", dict(contiguous=False, deal="tiles", deal_group=0)),
                 ("block_rows_round_robin", dict(contiguous=False, deal="rows", deal_group=0)),
                 ("contiguous_bands", dict(contiguous=False, deal="bands", deal_group=0)))
        for N in (2, 4, 8):
            row = {}
            for name, kw in deals:
                a = argparse.Namespace(**dict(vars(args), **kw))
                ms, kms, rays = [], [], []
                ms_pair = []
                for r in range(N):
                    fb = FrameBench(argparse.Namespace(**dict(vars(a), frame_pair=0)), None, device, N, r, None, renderer=rend)
                    fb.step()
                    evs, timing = [], []
                    for _ in range(steps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fb.step(timing)
                        e1.record()
                        evs.append((e0, e1))
                    torch.cuda.synchronize()
                    per = sorted(e0.elapsed_time(e1) for e0, e1 in evs)
                    k = kernel_ms(timing, steps)
                    ms.append(per[len(per) // 2])
                    kms.append([k.get("render_march", 0.0), k.get("render_shade", 0.0)])
                    rays.append(sum(n for _, n in timing) // steps)
                    del fb
                    # the same share with consecutive frames on two streams / two work lists (--frame-pair): frames per second of a
                    # continuously fed rank, GPU time of 2 x steps back-to-back frames between two events that bracket BOTH streams
                    fbp = FrameBench(argparse.Namespace(**dict(vars(a), frame_pair=1)), None, device, N, r, None, renderer=rend)
                    if fbp.pair is not None:
                        fbp.step(); fbp.step()
                        torch.cuda.synchronize()
                        main = torch.cuda.current_stream(device)
                        batches = []
                        for _ in range(3):             # median of three batches (an idle -> busy start-up glitch of 25-80 ms hits ~5 % of batches)
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record(main)
                            for st in fbp.pair:
                                st.wait_event(e0)
                            for _ in range(2 * steps):
                                fbp.step()
                            for st in fbp.pair:
                                main.wait_stream(st)
                            e1.record(main)
                            torch.cuda.synchronize()
                            batches.append(e0.elapsed_time(e1) / (2 * steps))
                        ms_pair.append(sorted(batches)[1])
                    rend.use_workspace_slot(0)
                    del fbp
                row[name] = {"share_ms": [round(x, 4) for x in ms], "share_march_shade_ms": [[round(x, 4) for x in p] for p in kms], "share_rays": rays,
                             "slowest_share_ms": max(ms), "mean_share_ms": sum(ms) / N,
                             "predicted_speedup": t1_ms / max(ms), "predicted_efficiency": t1_ms / (N * max(ms)),
                             "imbalance_max_over_mean": max(ms) / (sum(ms) / N)}
                if len(ms_pair) == N:
                    row[name].update({"frame_pair_share_ms": [round(x, 4) for x in ms_pair], "frame_pair_slowest_share_ms": max(ms_pair),
                                      "frame_pair_predicted_speedup": t1p / max(ms_pair),
                                      "frame_pair_predicted_efficiency": t1p / (N * max(ms_pair))})
            out["N=%d" % N] = row
        return out
    except Exception as e:          # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, e)}


def truck_render_block(args, device, want_cpu):
    """BASELINE.json configs[2]'s RENDER half at its real shape (VERDICT r4 "missing" #1): truck_single.py's model
    (configs/tankstemple_unbounded/truck_single.py:92-110: fourier_freq_num = 4 -> P = 9 levels, G = 200^3 for both grids, rgbnet_dim 12,
    viewbase_pe 4, stepsize 0.5 -> S = 668, fast_color_thres 1e-4) through the frame loop of run_render.py:54-66 -- one 1920x1080 view,
    trained-like synthetic fields (make_state_surfaces with F = 4; 30 GB of bricks).  F >= 4 takes another shade geometry than the
    headline (8 waves: 4 producers + 4 consumers, csrc/ugrid_shade.hip ug_shade_launch), so this leg is also that kernel's only
    frame-scale clock.  Reports ms per frame, per-kernel times, survivors and the parity of 4 x 8192 rays spread over the frame against
    the CPU oracle.  Secondary: a failure here never costs the headline line."""
    try:
        F, G = 4, args.grid
        t_args = argparse.Namespace(**dict(vars(args), stepsize=0.5, freq=F))
        state = make_state_surfaces(G, device, seed=0, F=F)
        fb = FrameBench(t_args, state, device, 1, 0, None)
        cpu_state = None
        if want_cpu:
            cpu_state = {k: ([x.cpu() for x in v] if isinstance(v, list) else (v.cpu() if torch.is_tensor(v) else v)) for k, v in state.items()}
        del state
        torch.cuda.empty_cache()
        steps = max(4, args.steps // 2)
        dt, kern, dt1 = timed_with_kernels(fb, steps, 1)
        rays, out, M = fb.full_frame()
        R, S, P = fb.R, fb.S, 1 + 2 * F
        t = dt / steps
        alg = {"render_march": R * S * 32 * P + R * 32, "render_shade": M * 384 * P + R * 24}
        res = {"workload": "truck_single.py-shaped render: F = 4 (P = 9), G = %d^3, C = 12, rgbnet 39-128-128-3, stepsize 0.5 -> S = %d, thres 1e-4, "
                           "%dx%d rays, trained-like synthetic fields (make_state_surfaces)" % (G, S, fb.W, fb.H),
               "value": R * S / t / 1e6, "unit": "Msamples/s", "ms_per_step": t * 1e3, "steps": steps, "rays_per_sec": R / t,
               "frames_in_flight": len(fb.pair) if fb.pair is not None else 1, "ms_per_step_single_stream": (dt1 / steps * 1e3) if dt1 else None,
               "samples_per_ray": S, "survivors_M": M, "survivor_frac": M / float(R * S),
               "terminated_ray_frac": float((out["alphainv_last"] < 1e-3).float().mean()),
               "kernels": {k: {"ms": v, "algorithmic_bytes": alg.get(k), "algorithmic_GBps": (alg[k] / (v * 1e-3) / 1e9) if k in alg and v > 0 else None}
                           for k, v in kern.items()},
               "shade_kernel": "k_shade_pc<4,4,6,2,3,1,true> (12 waves: 6 gather + 6 rgbnet; F >= 4 enters the 12-wave geometry through the rolling cell set-up)"}
        if cpu_state is not None:
            cb = cpu_baseline(cpu_state, rays, out, fb.stepsize, S, 4, device, ref_gpu=False)
            res["cpu_baseline_Msamples"] = cb["value"]
            res["cpu_baseline_kind"] = cb["kind"]
            res["gpu_vs_oracle"] = cb["gpu_vs_oracle"]
        del fb, out, rays
        torch.cuda.empty_cache()
        return res
    except Exception as e:          # noqa: BLE001
        torch.cuda.empty_cache()
        return {"error": "%s: %s" % (type(e).__name__, e)}


def voxgo_train_block():
    """Row f4 of SURVEY section 8 under the driver's clock: one training step of voxgo_model.DirectVoxGO at the lego fine-stage
    shape (the model of BASELINE.json configs[0]) and of DirectContractedVoxGO at the Mip-360 fine-stage shape (configs[1]'s model),
    tools/bench_voxgo_train.run.  Secondary: a failure here never costs the headline line."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import argparse
        import bench_voxgo_train as bvt
        a = argparse.Namespace(steps=45, warmup=8, blocks=3, grid=0, fused=1, overlap=1, lazy_loss=0, native=1)      # (8 warm-up steps: the first launches of the backward kernels load their code objects)
        out = {}
        for kind, first, tag in (("dvgo", 1, "dvgo_lego_fine"), ("dcvgo", 1, "dcvgo_mip360_fine_dense_tv"), ("dcvgo", 10001, "dcvgo_mip360_fine_masked_tv")):
            r = bvt.run(kind, a, first)
            out[tag] = {k: r[k] for k in ("workload", "native_step", "ms_per_step", "rays_per_sec", "survivors_M", "steps")}
            torch.cuda.empty_cache()
        # round 6: no host read in the loop (sync-free native step + the loss as a tensor), the two steps VERDICT r5 item 5 / 6 name
        b = argparse.Namespace(**dict(vars(a), lazy_loss=1, sync_free=1))
        for kind, first, tag in (("dvgo", 1, "dvgo_lego_fine_sync_free"), ("dcvgo", 10001, "dcvgo_mip360_fine_masked_tv_sync_free")):
            r = bvt.run(kind, b, first)
            out[tag] = {k: r[k] for k in ("workload", "native_step", "sync_free", "lazy_loss", "ms_per_step", "rays_per_sec", "survivors_M", "steps")}
            torch.cuda.empty_cache()
        return out
    except Exception as e:          # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, e)}


def voxgo_render_block(steps):
    """BASELINE.json configs[0] / configs[1] as worded, the RENDER halves: one DirectVoxGO view of the lego box at 800 x 800 (160^3) and one
    DirectContractedVoxGO 1080p frame (320^3, S = 1068) through the fused renderers -- tools/bench_dvgo.py, tools/bench_dcvgo.py: ms per view on
    one stream and with two / four views in flight (run_render.render_viewpoints), agreement with the composed forward.  Secondary."""
    res = {}
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_dcvgo
        import bench_dvgo
        d = bench_dvgo.main(["--steps", str(max(10, steps))], quiet=True)
        n4 = (d.get("ms_n_in_flight") or {}).get("4")
        res["dvgo_lego_800_view"] = dict(d, ms_per_step=n4 or d["ms_per_view_two_in_flight"], frames_in_flight=4 if n4 else 2,
                                         ms_per_step_single_stream=d["ms_per_view"])
        torch.cuda.empty_cache()
        c = bench_dcvgo.main(["--steps", str(max(5, steps // 2))], quiet=True)
        res["dcvgo_1080p_frame"] = dict(c, ms_per_step=c["ms_per_frame_two_in_flight"], frames_in_flight=2, ms_per_step_single_stream=c["ms_per_frame"])
        torch.cuda.empty_cache()
    except Exception as e:          # noqa: BLE001
        torch.cuda.empty_cache()
        res["error"] = "%s: %s" % (type(e).__name__, e)
    return res


def self_launch(args):
    """`python bench.py --gpus N` without a launcher (WORLD_SIZE unset): start the N ranks ourselves through
    torch.distributed.run on 127.0.0.1 -- the command the driver uses for N > 1 -- and pass their exit code on.  On a box
    with fewer than N GPUs the run is refused unless UGRID_BENCH_SHARE_GPU=1 (debugging: all ranks on the devices there
    are, over gloo, since RCCL refuses two ranks on one device)."""
    import socket
    import subprocess
    env = os.environ.copy()
    standin = env.get("UGRID_BENCH_STANDIN")
    ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if not standin and ndev < args.gpus:
        if env.get("UGRID_BENCH_SHARE_GPU") != "1" or ndev == 0:
            raise SystemExit("bench.py --gpus %d needs %d MI355X (found %d); UGRID_BENCH_SHARE_GPU=1 runs the ranks on the devices "
                             "present over gloo (debugging only)" % (args.gpus, args.gpus, ndev))
        env.setdefault("UGRID_BENCH_BACKEND", "gloo")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def _standin_renderer(spec):
    """UGRID_BENCH_STANDIN=module:factory (CI only, tests/test_host_logic.py): a stand-in with the renderer's call
    signature on the CPU, so that the launch / sharding / exchange / assembly logic of this file runs without a GPU.  The
    JSON line then says "renderer": "stand-in" and carries no roofline / cpu_baseline -- it is not a measurement."""
    import importlib
    mod, fn = spec.split(":")
    return getattr(importlib.import_module(mod), fn)()


def headline(args, fb, dt, world, use_dist, n_chunks, standin):
    """The headline figures of the K timed steps (`dt` seconds): all a plain run reports; --full adds its blocks to this dict."""
    R, S, G = fb.R, fb.S, args.grid
    scene_desc = {"s1": "white-noise grids N(%g,%g^2)" % (DENS_MEAN, DENS_STD),
                  "s1b": "smooth fields with opaque surfaces (make_state_surfaces)"}
    res = {
        "metric": "Msamples/sec (Mip-360 garden-shaped 1920x1080x256 frame, FourierGrid render)",
        "value": R * S / (dt / args.steps) / 1e6, "unit": "Msamples/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "rays_per_sec": R / (dt / args.steps),
        "frames_in_flight": len(fb.pair) if fb.pair is not None else 1,
        "config": {"workload": "%s %dx%dx%d G%d F%d(P%d) C12 rgbnet 39-128-128-3 f32 stepsize %.3g thres 1e-4 %s"
                               % (args.scene.upper(), fb.W, fb.H, S, G, args.freq, 1 + 2 * args.freq, fb.stepsize,
                                  {"s1": "white-noise grids", "s1b": "trained-like fields"}[args.scene]),
                   "workload_long": "%s: FourierGridModel render, R=%dx%d rays x S=%d samples, G=%d^3, F=%d (P=%d), C=12, "
                                    "rgbnet 39-128-128-3, stepsize %.3g, thres 1e-4, %s"
                                    % (args.scene.upper(), fb.W, fb.H, S, G, args.freq, 1 + 2 * args.freq, fb.stepsize, scene_desc[args.scene]),
                   "rays": R, "samples_per_ray": S, "chunks_per_frame": n_chunks,
                   "step": "ray generation + march + shade + %s%s" % (
                       "all-gather of the tiles + frame assembly (un-deal, un-tile)" if use_dist else "un-tiling to image order",
                       "; %d frames in flight" % len(fb.pair) if fb.pair is not None else ""),
                   "ray_order": "shuffled (incoherent tiles)" if args.shuffle_rays else (
                       "%dx%d pixel blocks (one 8x8 block per 64-ray wave), results back in image order" % (args.ray_tile, args.ray_tile)
                       if fb.order is not None else "image order (64-pixel row segments per wave)"),
                   "parallelism": ("one frame over %d ranks, %s, 1 all-gather of [R/N,5] tiles per frame (async, overlaps "
                                   "the next frame)" % (world, "contiguous 64-aligned ray bands" if fb.contiguous
                                                        else "64-ray tiles (8x8 pixel blocks) dealt round-robin in groups of %d" % fb.deal_group))
                                   if world > 1 else "1 GPU"},
    }
    if standin:
        res["renderer"] = "stand-in (%s): CI run of the launch / exchange / assembly logic, NOT a measurement" % standin
    else:
        res["lib_sha16"] = lib_sha16()
        res["device_code_sha16"] = device_code_sha16()
    return res


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1 and "RANK" not in os.environ:
            raise SystemExit(self_launch(args))
        raise SystemExit("WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))
    standin = os.environ.get("UGRID_BENCH_STANDIN")
    if standin:
        device = torch.device("cpu")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X (no CPU fallback for the measured path)")
        # UGRID_BENCH_SHARE_GPU=1 (debugging only): all ranks on the devices present, e.g. two gloo ranks on a single-GPU box
        # to exercise the multi-rank frame path (tile dealing, exchange, frame assembly) on the real renderer
        if os.environ.get("UGRID_BENCH_SHARE_GPU") == "1":
            local_rank = local_rank % torch.cuda.device_count()
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    dist = None
    use_dist = world > 1 or ("RANK" in os.environ and os.environ.get("UGRID_BENCH_FORCE_DIST") == "1")
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        backend = os.environ.get("UGRID_BENCH_BACKEND", "gloo" if standin else "nccl")   # "nccl" = RCCL; gloo: debugging / CI
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    if not standin:
        from unboundednerfpytorch_amd.fourier_render import tune
        for kv in args.tune:
            k, v = kv.split("=")
            tune(k, int(v))

    make = {"s1": make_state, "s1b": make_state_surfaces}
    G = args.grid
    if standin:
        state = None
        fb = FrameBench(args, None, device, world, rank, dist, renderer=_standin_renderer(standin))
    else:
        state = make[args.scene](G, device, seed=0, F=args.freq)  # same model on every rank (replicated read-only grids)
        fb = FrameBench(args, state, device, world, rank, dist)
    want_cpu = args.full and rank == 0 and not args.no_cpu_baseline and not standin
    cpu_state = None
    if want_cpu:
        cpu_state = {k: ([x.cpu() for x in v] if isinstance(v, list) else (v.cpu() if torch.is_tensor(v) else v))
                     for k, v in state.items()}
    del state
    if not standin:
        torch.cuda.empty_cache()

    dt, timing = fb.timed(args.steps, args.warmup)
    if args.dump_outputs and rank == 0:
        dump_outputs(fb, args.dump_outputs)
    if not args.full:
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        if rank == 0:
            res = headline(args, fb, dt, world, use_dist, len(timing) // max(1, args.steps), standin)
            print(json.dumps(compact_line(res, detail=False), separators=(",", ":")))
        return
    fb.check_exchange()
    # with two frames in flight (the stream pair, default) the march of frame k + 1 runs beside the shade of frame k: the HIP-event duration
    # of a launch then includes its neighbour's work.  The per-kernel durations (`kernels`, `roofline`) come from a SECOND timed region of the
    # same K steps on one stream, every launch alone on the chip -- the regime `rocprofv3 --stats` of `bench.py --frame-pair 0` reproduces.
    dt_single = None
    if fb.pair is not None:
        dt_single, timing = fb.timed(args.steps, 1, single_stream=True)
    kern = kernel_ms(timing, args.steps)
    n_chunks = len(timing) // max(1, args.steps)
    rays_this_rank = sum(n for _, n in timing) // max(1, args.steps)
    M_rank = fb.rend.survivors_of_last_chunk() if (not standin and n_chunks == 1) else None
    # per-rank kernel times (load imbalance of the strong-scaled frame)
    per_rank = None
    if use_dist:
        mine = torch.tensor([kern.get("render_march", 0.0), kern.get("render_shade", 0.0),
                             float(rays_this_rank)], device=device, dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [{"rank": i, "march_ms": float(a[0]), "shade_ms": float(a[1]), "rays": int(a[2])} for i, a in enumerate(allr)]
    weak = None
    if use_dist and world > 1:
        wdt, _ = fb.timed(max(3, args.steps // 2), 1, weak=True)
        wsteps = max(3, args.steps // 2)
        weak = {"value": world * fb.R * fb.S / (wdt / wsteps) / 1e6, "unit": "Msamples/s", "ms_per_step": wdt / wsteps * 1e3,
                "note": "every rank renders its own full frame (own camera); no exchange"}
    proxy = None
    if world == 1 and not use_dist and not standin and not args.no_proxy and args.height % 8 == 0 and args.width % 8 == 0:
        proxy = scaling_proxy(args, fb.rend, device, (dt_single or dt) / args.steps * 1e3, t1_pair_ms=dt / args.steps * 1e3 if dt_single else None)
    # survivor statistics + parity inputs from one extra, untimed full frame on this rank
    rays_full, out_full, M = fb.full_frame()
    R, S = fb.R, fb.S
    # self-check of the strong-scaled path: the frame assembled from all ranks' tiles INSIDE the timed step must be, bit
    # for bit, the frame one rank renders on its own (per-ray results do not depend on which rank or wave rendered them)
    frame_ok = None
    if use_dist:
        asm = fb.assembled_frame()
        frame_ok = bool(torch.equal(asm[:, 0:3], out_full["rgb_marched"]) and torch.equal(asm[:, 3], out_full["depth"])
                        and torch.equal(asm[:, 4], out_full["alphainv_last"]))
        if world > 1:
            ok_all = torch.tensor([1.0 if frame_ok else 0.0], device=device)
            dist.all_reduce(ok_all, op=dist.ReduceOp.MIN)
            frame_ok = bool(ok_all.item() > 0)
    term_frac = float((out_full["alphainv_last"] < 1e-3).float().mean())
    # sha256 over the bytes of the frame (rgb, depth, alphainv_last): per-ray results are bitwise independent of the kernel
    # geometry, chunking and rank layout, so two builds that claim "same arithmetic" must print the same value
    frame_sha = None
    if rank == 0 and not standin:
        import hashlib
        hh = hashlib.sha256()
        for k_ in ("rgb_marched", "depth", "alphainv_last"):
            hh.update(out_full[k_].contiguous().cpu().numpy().tobytes())
        frame_sha = hh.hexdigest()[:16]
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()     # everything below is rank 0's own (CPU baseline: the other ranks are done)

    res = None
    if rank == 0:
        ms_step = dt / args.steps * 1e3
        res = headline(args, fb, dt, world, use_dist, n_chunks, standin)
        res["ms_per_step_single_stream"] = (dt_single / args.steps * 1e3) if dt_single else None
        res["config"].update({"survivors_M": M, "survivor_frac": M / float(R * S), "terminated_ray_frac": term_frac})
        res["kernels"] = {k: {"ms": v} for k, v in kern.items()}
        if standin:
            res["roofline"] = None
        else:
            res["frame_sha16"] = frame_sha
            if M_rank is not None:
                # rank 0's own kernels: its share of the frame's rays and survivors (the whole frame at N = 1)
                shade_passes = (M_rank + 31) // 32 + rays_this_rank // 64 // 2      # ~ sum over tiles of ceil(count / 32)
                default_s1 = (args.scene == "s1" and args.freq == 3 and not args.stepsize and G == 200 and (fb.H, fb.W) == (1080, 1920)
                              and not args.shuffle_rays and args.ray_tile == 8)
                res["roofline"] = roofline_block(kern, M_rank, rays_this_rank, S, shade_passes, frame_rays=R, P=1 + 2 * args.freq,
                                                 ms_per_step=((dt_single / args.steps * 1e3) if dt_single else ms_step) if world == 1 else None,
                                                 pmc_workload_ok=default_s1)
                if dt_single and isinstance(res["roofline"], dict):
                    res["roofline"]["region"] = "single_stream"
            else:
                res["roofline"] = None
        if proxy is not None:
            res["scaling_proxy"] = proxy
        if per_rank is not None:
            res["per_rank"] = per_rank
        if frame_ok is not None:
            res["assembled_frame_equals_single_rank_frame"] = frame_ok
        if weak is not None:
            res["weak_scaling"] = weak
        if cpu_state is not None:
            try:
                res["cpu_baseline"] = cpu_baseline(cpu_state, rays_full, out_full, fb.stepsize, S, args.cpu_chunks, device)
            except Exception as e:          # noqa: BLE001  (the measurement above stands on its own)
                res["cpu_baseline"] = {"error": "%s: %s" % (type(e).__name__, e)}
    # secondary scene (single GPU only: it re-packs 23 GB of bricks)
    if world == 1 and not use_dist and not args.no_secondary and args.scene == "s1" and not standin:
        del fb, out_full, rays_full
        cpu_state = None
        torch.cuda.empty_cache()
        sec_args = argparse.Namespace(**vars(args))
        state = make_state_surfaces(G, device, seed=0)
        fb2 = FrameBench(sec_args, state, device, 1, 0, None)
        cpu2 = None
        if want_cpu:
            cpu2 = {k: ([x.cpu() for x in v] if isinstance(v, list) else (v.cpu() if torch.is_tensor(v) else v))
                    for k, v in state.items()}
        del state
        torch.cuda.empty_cache()
        steps2 = max(3, args.steps // 2)
        dt2, kern2, dt2s = timed_with_kernels(fb2, steps2, 1)
        rays2, out2, M2 = fb2.full_frame()
        sec = {"workload": "S1b: same model shape, smooth fields with opaque surfaces (make_state_surfaces)",
               "value": fb2.R * fb2.S / (dt2 / steps2) / 1e6, "unit": "Msamples/s", "ms_per_step": dt2 / steps2 * 1e3, "steps": steps2,
               "ms_per_step_single_stream": (dt2s / steps2 * 1e3) if dt2s else None,
               "survivor_frac": M2 / float(fb2.R * fb2.S), "terminated_ray_frac": float((out2["alphainv_last"] < 1e-3).float().mean()),
               "kernels": {k: {"ms": v} for k, v in kern2.items()}}
        res["secondary"] = sec
        # the SAME trained-like scene at garden_single.py's own sampling (configs/nerf_unbounded/garden_single.py:8-21: stepsize 0.5,
        # fast_color_thres 1e-4 from iteration 6500 on -> S = 668 samples per ray at G = 200).  The headline metric is quoted on the
        # 256-sample frame (BASELINE.json); this is what one frame of the real config costs (VERDICT r3 "missing" #7).
        try:
            g_args = argparse.Namespace(**dict(vars(args), stepsize=0.5))
            fb3 = FrameBench(g_args, None, device, 1, 0, None, renderer=fb2.rend)       # same packed bricks
            steps3 = max(4, args.steps // 2)
            dt3, kern3, dt3s = timed_with_kernels(fb3, steps3, 1)
            _, out3, M3 = fb3.full_frame()
            res["secondary_garden_single_sampling"] = {
                "workload": "S1b scene at garden_single.py's sampling: stepsize 0.5 -> S = %d samples per ray, fast_color_thres 1e-4" % fb3.S,
                "value": fb3.R * fb3.S / (dt3 / steps3) / 1e6, "unit": "Msamples/s", "ms_per_step": dt3 / steps3 * 1e3, "steps": steps3,
                "ms_per_step_single_stream": (dt3s / steps3 * 1e3) if dt3s else None,
                "rays_per_sec": fb3.R / (dt3 / steps3), "samples_per_ray": fb3.S, "survivor_frac": M3 / float(fb3.R * fb3.S),
                "terminated_ray_frac": float((out3["alphainv_last"] < 1e-3).float().mean()),
                "kernels": {k: {"ms": v} for k, v in kern3.items()}}
            del fb3, out3
        except Exception as e:          # noqa: BLE001  (a secondary must never cost the headline line)
            res["secondary_garden_single_sampling"] = {"error": "%s: %s" % (type(e).__name__, e)}
        # (the CPU baseline of the S1b frame runs AFTER every GPU timing of this renderer: a minute of 8-thread host work right
        # before a timed loop left the loop host-bound in one run, 14.2 instead of 11.9 ms per S = 668 frame)
        if cpu2 is not None:
            cb = cpu_baseline(cpu2, rays2, out2, fb2.stepsize, fb2.S, max(4, args.cpu_chunks // 2), device, ref_gpu=False)
            sec["cpu_baseline_Msamples"] = cb["value"]
            sec["gpu_vs_oracle"] = cb["gpu_vs_oracle"]
        del out2, rays2
        del fb2
        torch.cuda.empty_cache()
        if not args.no_truck and args.height == 1080 and args.width == 1920:
            res["secondary_truck_render"] = truck_render_block(args, device, want_cpu)
        s3 = s3_train_step_block(device)
        if s3 is not None:
            res["secondary_s3_train_step"] = s3
            if isinstance(s3.get("roofline_tv_adam_dense"), dict):
                res["roofline_hbm"] = hbm_roofline_entry(s3["roofline_tv_adam_dense"])
        res["secondary_voxgo_train_steps"] = voxgo_train_block()
        res["secondary_voxgo_renders"] = voxgo_render_block(args.steps)
    if rank == 0:
        line = compact_line(res)
        print(json.dumps(line, separators=(",", ":")))


LINE_BUDGET = 4096          # bytes: the driver parses the LAST stdout line; a 22 KB line (round 5) did not parse


def _num(x, nd=4):
    """a float rounded to nd significant digits (the detail file keeps full precision); everything else unchanged"""
    if isinstance(x, float) and math.isfinite(x) and x != 0.0:
        return float("%.*g" % (nd, x))
    return x


def _pick(d, keys, nd=4):
    return {k: _num(d.get(k), nd) for k in keys if isinstance(d, dict) and k in d}


def write_detail(res, path=None):
    """Everything bench.py measured (per-kernel blocks, fp64 ground truth, arbitration, scaling_proxy, per-output parity statistics of
    the secondaries) goes to bench_detail.json next to this file -- and, on a gpurun box, to gpurun_out/ so that it travels back.
    Returns (path relative to the repo, sha16 of the bytes)."""
    blob = json.dumps(res, indent=1, sort_keys=True).encode()
    path = path or os.environ.get("UGRID_BENCH_DETAIL") or os.path.join(ROOT, "bench_detail.json")
    try:
        with open(path, "wb") as f:
            f.write(blob)
        out_dir = os.path.join(ROOT, "gpurun_out")
        if os.path.isdir(out_dir) and os.path.dirname(os.path.abspath(path)) == ROOT:
            with open(os.path.join(out_dir, os.path.basename(path)), "wb") as f:
                f.write(blob)
    except OSError as e:            # a read-only tree must not cost the line
        return {"path": None, "error": str(e), "sha16": hashlib.sha256(blob).hexdigest()[:16], "bytes": len(blob)}
    return {"path": os.path.relpath(path, ROOT), "sha16": hashlib.sha256(blob).hexdigest()[:16], "bytes": len(blob)}


def compact_line(res, detail_path=None, detail=True):
    """The ONE line the driver parses: the contract's keys, `roofline` / `roofline_hbm` / `cpu_baseline` as numbers only, one
    number (ms per step) per secondary, and where the rest went (`detail`: bench_detail.json + its sha16; detail=False: a plain
    run's line, no file).  Always < LINE_BUDGET bytes (tests/test_host_logic.py::test_bench_line_fits_the_driver)."""
    line = {k: _num(res.get(k), 6) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                             "scaling", "vs_baseline", "dtype", "data", "rays_per_sec", "frames_in_flight",
                                             "ms_per_step_single_stream") if k in res}
    cfg = res.get("config") or {}
    line["config"] = {"workload": str(cfg.get("workload", ""))[:119]}
    line["config"].update(_pick(cfg, ("rays", "samples_per_ray", "survivors_M", "survivor_frac", "chunks_per_frame")))
    line["config"]["parallelism"] = str(cfg.get("parallelism", ""))[:60]
    line["config"]["step"] = str(cfg.get("step", ""))[:100]
    if "kernels" in res:
        line["kernels"] = {k: _num(v.get("ms")) for k, v in (res.get("kernels") or {}).items()}
    for k in ("renderer", "lib_sha16", "device_code_sha16", "frame_sha16", "assembled_frame_equals_single_rank_frame"):
        if k in res:
            line[k] = res[k]
    rf = res.get("roofline")
    if isinstance(rf, dict):
        line["roofline"] = _pick(rf, ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "ta_busy_measured", "hbm_frac_measured",
                                      "frac_of_hbm_algorithmic", "region"))
        pk = rf.get("per_kernel") or {}
        line["roofline"]["per_kernel"] = {k: _pick(v, ("ms", "l1_frac", "hbm_frac", "mfma_frac", "ta_busy_measured", "mfma_pipe_busy", "valu_issue_busy",
                                                       "rocprofv3_avg_ms"), 3) for k, v in pk.items()}
    elif "roofline" in res:
        line["roofline"] = None
    rh = res.get("roofline_hbm")
    if isinstance(rh, dict):
        line["roofline_hbm"] = _pick(rh, ("kernel", "bound", "achieved", "peak", "unit", "frac", "ms", "algorithmic_bytes", "traffic"))
    cb = res.get("cpu_baseline")
    if isinstance(cb, dict):
        if "error" in cb:
            line["cpu_baseline"] = {"error": str(cb["error"])[:200]}
        else:
            c = _pick(cb, ("value", "unit", "cores", "host_cores", "kind"))
            c["sample"] = str(cb.get("sample", ""))[:60]
            c["linf"] = {"rgb": _num(cb.get("gpu_vs_oracle_linf_rgb"), 3), "depth": _num(cb.get("gpu_vs_oracle_linf_depth"), 3),
                         "alphainv_last": _num(cb.get("gpu_vs_oracle_linf_alphainv_last"), 3)}
            line["cpu_baseline"] = c
    if isinstance(res.get("weak_scaling"), dict):
        line["weak_scaling"] = _pick(res["weak_scaling"], ("value", "unit", "ms_per_step"))
    # one number per secondary: ms per step (a frame or a training step); the workloads are named in DESIGN.md / the detail file
    sec = {}

    def put(name, d, *path):
        for k in path:
            d = d.get(k) if isinstance(d, dict) else None
        if isinstance(d, dict) and "error" in d:
            sec[name] = "error"
        elif isinstance(d, dict) and "ms_per_step" in d:
            sec[name] = _num(d["ms_per_step"])
    put("s1b_render", res.get("secondary"))
    put("s1b_s668_render", res.get("secondary_garden_single_sampling"))
    put("truck_render", res.get("secondary_truck_render"))
    for name, key in (("s1b_render_1stream", "secondary"), ("truck_render_1stream", "secondary_truck_render")):
        d = res.get(key)
        if isinstance(d, dict) and d.get("ms_per_step_single_stream"):
            sec[name] = _num(d["ms_per_step_single_stream"])
    tr = res.get("secondary_truck_render")
    if isinstance(tr, dict) and isinstance(tr.get("kernels"), dict):
        for k, v in tr["kernels"].items():
            sec["truck_" + k.replace("render_", "")] = _num(v.get("ms"))
        g = tr.get("gpu_vs_oracle") or {}
        if g:
            sec["truck_linf_rgb"] = _num((g.get("rgb_marched") or {}).get("linf_all"), 3)
    s1b = res.get("secondary")
    if isinstance(s1b, dict) and isinstance(s1b.get("kernels"), dict):
        sec["s1b_shade"] = _num((s1b["kernels"].get("render_shade") or {}).get("ms"))
    put("s3_train_dense_tv", res.get("secondary_s3_train_step"), "dense_tv")
    put("s3_train_masked_tv", res.get("secondary_s3_train_step"), "masked_tv")
    put("s3_train_masked_tv_sync_free", res.get("secondary_s3_train_step"), "masked_tv_sync_free")
    vg = res.get("secondary_voxgo_train_steps")
    if isinstance(vg, dict):
        if "error" in vg:
            sec["voxgo_train"] = "error"
        for k in vg:
            put(k, vg, k)
    vr = res.get("secondary_voxgo_renders")
    if isinstance(vr, dict):
        if "error" in vr:
            sec["voxgo_render"] = "error"
        for k in ("dvgo_lego_800_view", "dcvgo_1080p_frame"):
            put(k, vr, k)
            if isinstance(vr.get(k), dict) and vr[k].get("ms_per_step_single_stream"):
                sec[k + "_1stream"] = _num(vr[k]["ms_per_step_single_stream"])
    if sec:
        line["secondary_ms"] = sec
    px = res.get("scaling_proxy")
    if isinstance(px, dict) and isinstance(px.get("N=8"), dict):
        b = px["N=8"].get("contiguous_bands") or {}
        line["scaling_proxy_N8"] = _pick(b, ("slowest_share_ms", "predicted_speedup", "frame_pair_slowest_share_ms", "frame_pair_predicted_speedup"))
    if detail:
        line["detail"] = write_detail(res, detail_path)
    n = len(json.dumps(line, separators=(",", ":")))
    if n >= LINE_BUDGET:            # never print an unparseable line: drop the optional blocks, largest first
        for k in ("secondary_ms", "scaling_proxy_N8", "weak_scaling", "roofline_hbm"):
            line.pop(k, None)
            if len(json.dumps(line, separators=(",", ":"))) < LINE_BUDGET:
                break
    return line


def cpu_baseline(cpu_state, rays, gpu_out, stepsize, S, n_chunks, device=None, ref_gpu=True):
    """The CPU baseline timed on this box's host cores on a bounded sample of the same frame (n_chunks x 8192 rays spread
    over the image), and the parity of the GPU frame against it.

    kind "reference" (whenever the reference's Python is present -- /root/reference in the build
    container, the git-ignored archive oracle/_ref/reference_py.tar on the GPU box): the reference's OWN
    FourierGridModel.forward (FourierGrid_model.py:554-672, pure-PyTorch F.grid_sample path) in its own 8192-ray render
    chunks, its four CUDA-only extension modules served by the C restatement (oracle/ref_ops.c; the reference has no CPU
    build of them).  kind "port" otherwise: oracle/model_oracle.py, the torch-CPU restatement pinned bit for bit on that
    Python.  With oracle/_ref present (ref_gpu) the same rays also go through the reference executing on THIS GPU -- its
    Python over its own compiled kernels -- and the three pairwise L-inf are reported (`arbitration`)."""
    from oracle import model_oracle, ref_model
    # torch's intra-op threading stops scaling early on this op mix: on the 256-core GPU-box host 8 threads
    # gave 8.6 Msamples/s, 64 -> 5.4, 256 -> 0.13 (tools/cpu_threads_sweep.py); use the fastest setting.
    cores = min(8, os.cpu_count() or 1)
    torch.set_num_threads(cores)
    ro, rd, vd = rays
    R = ro.shape[0]
    chunk = 8192
    starts = [int(i * (R - chunk) / max(1, n_chunks - 1)) // 64 * 64 for i in range(n_chunks)] if n_chunks > 1 else [0]
    kind = "reference" if ref_model.available("oracle") else "port"
    model = ref_model.reference_model(cpu_state, "cpu", "oracle") if kind == "reference" else None
    t_total, n_samples = 0.0, 0
    errs = {k: [] for k in ("rgb_marched", "depth", "alphainv_last")}
    refs = {k: [] for k in errs}
    margins, sq = [], 0.0
    for i, b in enumerate([starts[0]] + starts):  # first pass = warm-up, not timed
        o, d, v = ro[b:b + chunk].cpu(), rd[b:b + chunk].cpu(), vd[b:b + chunk].cpu()
        t0 = time.perf_counter()
        if model is not None:
            ref = ref_model.render(model, o, d, v, stepsize, chunk=chunk)
        else:
            ref = model_oracle.fouriergrid_render(cpu_state, o, d, v, stepsize, render_depth=True, return_margin=True)
        t1 = time.perf_counter()
        if i == 0:
            continue
        t_total += t1 - t0
        n_samples += chunk * S
        if model is not None:      # the threshold margins of the sampled rays come from the restatement (untimed)
            margins.append(model_oracle.fouriergrid_render(cpu_state, o, d, v, stepsize, render_depth=True, return_margin=True)["margin"])
        else:
            margins.append(ref["margin"])
        for k in errs:
            err = (gpu_out[k][b:b + chunk].cpu() - ref[k]).abs()
            errs[k].append(err.amax(dim=1) if err.dim() == 2 else err)
            refs[k].append(ref[k])
        sq += float(((gpu_out["rgb_marched"][b:b + chunk].cpu() - ref["rgb_marched"]).double() ** 2).sum())
    errs = {k: torch.cat(v) for k, v in errs.items()}
    stats = parity_stats(errs, torch.cat(margins), sq)
    out = {"value": n_samples / t_total / 1e6, "unit": "Msamples/s", "cores": cores, "host_cores": os.cpu_count(), "kind": kind,
           "sample": "%dx8192 rays x %d samples of the same frame, %d threads" % (n_chunks, S, cores),
           "sample_long": "%d chunks x 8192 rays x %d samples of the same frame (%s, torch CPU grid_sample path, %d threads: the "
                          "fastest setting on this host), 1 warm-up chunk"
                          % (n_chunks, S, "the reference's own FourierGridModel.forward over the C restatement of its extension modules"
                             if kind == "reference" else "oracle/model_oracle.py", cores),
           "rays_per_sec": n_chunks * chunk / t_total,
           "gpu_vs_oracle_linf_rgb": stats["rgb_marched"]["linf_all"], "gpu_vs_oracle_linf_depth": stats["depth"]["linf_all"],
           "gpu_vs_oracle_linf_alphainv_last": stats["alphainv_last"]["linf_all"],
           "gpu_vs_oracle": stats}
    del model
    rg = None
    if ref_gpu and device is not None and device.type == "cuda" and ref_model.available("kernels:fma"):
        try:
            out["arbitration"], rg = _arbitration(cpu_state, device, ro, rd, vd, starts, chunk, stepsize, gpu_out, refs)
        except Exception as e:          # noqa: BLE001  (the checker's checker must never cost the measurement line)
            out["arbitration"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if ref_gpu:
        # GROUND TRUTH: the rays where the fused frame is further than 1e-4 from a reference, plus 256 random
        # ones, re-evaluated in fp64 (tools/parity_fp64.py); the three distances to the truth and who is further from it how often
        try:
            sys.path.insert(0, ROOT)
            from tools import parity_fp64
            idx = torch.cat([torch.arange(b, b + chunk) for b in starts])
            evals = {"fused": {k: gpu_out[k].cpu()[idx] for k in refs}, "ref_cpu": {k: torch.cat(v) for k, v in refs.items()}}
            if rg is not None:
                evals["ref_gpu"] = rg
            gt = parity_fp64.ground_truth_study(cpu_state, (ro.cpu()[idx], rd.cpu()[idx], vd.cpu()[idx]), evals, stepsize, n_random=256, seed=0)
            gt.pop("per_ray", None)
            out["fp64_ground_truth"] = gt
        except Exception as e:          # noqa: BLE001
            out["fp64_ground_truth"] = {"error": "%s: %s" % (type(e).__name__, e)}
    return out


def _arbitration(cpu_state, device, ro, rd, vd, starts, chunk, stepsize, gpu_out, refs):
    """fused <-> the reference executing on this GPU <-> the reference on the CPU, L-inf over the sampled rays"""
    from oracle import ref_model
    gmodel = ref_model.reference_model(cpu_state, device, "kernels:fma")
    lin = lambda a, b: float(((a - b).abs().amax(dim=1) if a.dim() == 2 else (a - b).abs()).max())
    rg = {k: [] for k in refs}
    for b in starts:
        r = ref_model.render(gmodel, ro[b:b + chunk], rd[b:b + chunk], vd[b:b + chunk], stepsize, chunk=chunk)
        for k in rg:
            rg[k].append(r[k].cpu())
    del gmodel
    torch.cuda.empty_cache()
    idx = torch.cat([torch.arange(b, b + chunk) for b in starts])
    arb = {}
    for k in rg:
        g_ref, c_ref, fused = torch.cat(rg[k]), torch.cat(refs[k]), gpu_out[k].cpu()[idx]
        arb[k] = {"fused_vs_ref_on_gpu": lin(fused, g_ref), "ref_on_gpu_vs_ref_on_cpu": lin(g_ref, c_ref), "fused_vs_ref_on_cpu": lin(fused, c_ref)}
    return ({"note": "L-inf over the sampled rays; ref_on_gpu = the reference's own Python + its own compiled kernels (oracle/_ref/fma) + "
                     "torch-ROCm grid_sample on this MI355X", "rays": int(idx.numel()), **arb}, {k: torch.cat(v) for k, v in rg.items()})


def parity_stats(errs, margin, sq_rgb):
    """Per-output L-inf error against the oracle on the sampled rays: over ALL rays, and over the rays whose threshold
    margin exceeds m (smallest relative distance of any of the ray's samples to one of the three hard thresholds
    alpha > thres, weight > thres, T < 1e-3: a sample that sits on a threshold flips with ANY change of rounding and
    moves the ray by up to its weight).  `errs`: dict output -> per-ray error (a single tensor = already the max over
    the outputs, kept for old callers).  PSNR is over all sampled rays, flips included."""
    if torch.is_tensor(errs):
        errs = {"all_outputs": errs}
    n = margin.numel()
    out = {"rays": n, "psnr_rgb_db": 10.0 * math.log10(1.0 / max(sq_rgb / (3 * n), 1e-30)),
           "frac_rays_margin_gt_0.0001": float((margin > 1e-4).float().mean())}
    for k, err in errs.items():
        e = {"linf_all": float(err.max()), "mean_abs": float(err.mean()), "rays_above_1e-4": int((err > 1e-4).sum()),
             "frac_rays_above_1e-5": float((err > 1e-5).float().mean())}
        for m in (1e-4, 1e-3, 1e-2):
            sel = margin > m
            e["linf_margin_gt_%g" % m] = float(err[sel].max()) if bool(sel.any()) else None
        out[k] = e
    if "all_outputs" in out:         # flat layout of round 1 (tests/test_host_logic.py)
        flat = out.pop("all_outputs")
        out.update({"linf_all": flat["linf_all"], "mean_abs": flat["mean_abs"], "frac_rays_above_1e-5": flat["frac_rays_above_1e-5"]})
        for m in (1e-4, 1e-3, 1e-2):
            out["linf_margin_gt_%g" % m] = flat["linf_margin_gt_%g" % m]
            out["frac_rays_margin_gt_%g" % m] = float((margin > m).float().mean())
        out["note"] = "per-ray max over rgb, depth, alphainv_last"
    return out


if __name__ == "__main__":
    main()
