"""Hand-built scenes for the march half of the fused render -- ugrid_render_march (k_march, k_march_ring), ugrid_render_march_dcvgo
(k_march_dcvgo), ugrid_render_march_dvgo (k_march_dvgo), ugrid_render_march_mpi (k_march_mpi) -- and a plain torch reference of
each.  TEST INFRASTRUCTURE: tests/test_march_cases.py (CPU) checks this file, tests/test_gpu_march_worklist.py runs the kernels
on what it builds and reads their work lists (shade_cases.read_worklist).

The reference (march_reference) evaluates, for every (ray, step) and in float64 or float32, the formula of the reference
project's forward as include/ugrid_hip.h states it:

    fourier   p = contract((o - c) / r + d / |d| * t_j)                      density = mean over 1 + 2F levels of trilinear taps
    dcvgo     the same with the table of boundary 2; a contracted sample is evaluated only where the running inter-sample
              distance has passed dist_thres (cumdist_thres), and every sample only where the mask cache is set
    dvgo      p = o + d tmin + d / |d| * stepdist * j,  j < n = max(ceil((tmax - tmin) |d| / stepdist), 1); evaluated inside the box
              where the mask cache is set
    mpi       p = o + d * j / (n - 1), j < n; as dvgo, density = grid + the per-plane shift interpolated along z
    alpha = 1 - (1 + exp(density + shift)) ^ -interval;  a sample with alpha > thres composites (w = T alpha, T *= 1 - alpha,
    the ray ends once T < 1e-3) and SURVIVES -- is appended to its tile's work list as (p, w) -- when w > thres as well.
    depth = sum over survivors of w s_j | w j | w (j + 0.5) / n;  dcvgo: wsum_mid = sum of w over the un-contracted survivors.

float32 mode restates the oracle's own arithmetic (oracle/model_oracle.py, oracle/ref_ops.c raw2alpha, the float-state /
double-product transmittance scan) and is pinned on the golden vectors through it; float64 is the truth the kernels are held to.

The decision log.  The march takes discrete decisions; a kernel that is right to fp32 rounding may take another one than
float64 where the quantity sits on its threshold.  Every decision of every step is therefore logged with its distance to the
threshold, in the unit its error is measured in:
    alpha > thres, w > thres, T < 1e-3, cum > dist_thres, |p| <= 1 (dcvgo)       |q - thr| / max(|q|, thr)
    the mask cache's nearest-voxel rounding (when the neighbour it could flip to holds another value)   |frac - .5|, voxels
    outside-the-box (dvgo, mpi)                                                 distance to the nearest face / that axis's extent
    dvgo's step count ceil(x)                                                    |x - nearest integer >= 1|, steps
and e_dec = the largest float32-vs-float64 difference of that quantity on the case, in the same unit.  Every decision is held to
ITS error: a step is DECIDED when each of its decisions lies further than K * e_dec from its threshold, K = 8 (the kernel differs
from an fp32 evaluation by Markstein division, the brick polynomial, device sin / cos and ug_alpha, each worth about one such
error, times 2 for a maximum over a few thousand samples) -- or sits exactly ON the threshold in both precisions (an NDC ray's
first and last sample on the box faces: -2 + 3 * 0 and -2 + 3 * 1 involve no rounding).  The case's margin m is the widest of
them, K * max e_dec; tests/test_march_cases.py asserts m <= 1e-4, which the densities are chosen for (density_field).  A ray is
DECIDABLE when all the steps it ran are decided.  Undecidable rays are compared up to their first undecided step.

Value bounds: K * max(e32, floor) with e32 the reference's own float32 error of that output on the case; E32_LIMIT caps every e32.
"""
import functools
import math
import types

import numpy as np
import torch

from oracle import model_oracle, ref_ops
from shade_cases import GRID, BOX_LO, BOX_HI, SENTINEL, GUARD_ROWS, worklist_regions, read_worklist, rays_in_tile  # noqa: F401

K = 8.0
FLOOR = 2.0 ** -23
M_LIMIT = 1e-4                 # the margin tests/test_gpu_fused.py filters with
SET_ASIDE_LIMIT = 0.05         # check_render's cap on rays that may be set aside
# the largest e32 (absolute, float32 reference - float64 reference) of w / alphainv_last / depth / wsum_mid (units of 1) and of
# a position (units of the box extent) that tests/test_march_cases.py accepts on any case.  Measured on the CPU over all cases:
# w 6.9e-7, alphainv_last 6.9e-7, depth 1.1e-6 (dvgo: a sum of w * step index), wsum_mid 2.4e-7, positions 1.35e-7; the limits are
# those figures rounded up.
E32_LIMIT = {"w": 1e-6, "last": 1e-6, "depth": 2e-6, "wsum_mid": 5e-7, "pos": 2e-7}
PATTERN = 0xA5                 # the work list is filled with this byte before a march
VARIANTS = ("fourier", "dcvgo", "dvgo", "mpi")
THRES = 1e-4
G_FOURIER = 12
DCVGO_BOX = ([-0.9, -1.1, -1.0], [1.1, 0.9, 1.0])       # a cube (the contraction needs one) off the origin
DCVGO_WORLD_LEN = 12
DVGO_VOXEL = 0.25
EMPTY = -3e6                   # raw density of the empty voxels of `surfaces`
MASK_SHAPE = (6, 8, 10)
RAY_COUNTS = (5, 200, 64 * 5 + 3, 64 * 4 * 9 + 1)
SEEDS = {"surfaces": 1000, "capacity": 7, "mask": 5, "act_shift": 9}       # stated: tests/test_march_cases.py holds with these


# ---------------------------------------------------------------------------------------------------------------------
# host parameters, restated from fourier_render.FourierGridRenderer (tests/test_gpu_march_worklist.py compares with the renderer's)
# ---------------------------------------------------------------------------------------------------------------------
def variant_of(state):
    given = [n for n in ("dcvgo", "dvgo", "mpi") if state.get(n) is not None]
    return given[0] if given else "fourier"


def host_params(state, stepsize, near=0.0):
    """what the renderer hands the march entry point besides rays and grids: t / s tables, S, interval, the variant's scalars;
    every float is the fp32 value the C struct carries"""
    f32 = lambda x: float(np.float32(x))
    v = variant_of(state)
    h = types.SimpleNamespace(variant=v, t=None, s=None, near=f32(near))
    ratio = float(state["voxel_size_ratio"])
    if v == "mpi":
        D = int(state["density_grid"].shape[4])
        h.S = h.n = int((D - 1) / stepsize) + 1
        h.interval = f32(stepsize * ratio)
    else:
        h.interval = float(torch.tensor(ratio, dtype=torch.float32) * stepsize)
    if v == "dvgo":
        h.stepdist = float(stepsize * torch.as_tensor(state["dvgo"]["voxel_size"], dtype=torch.float32))
        ext = [float(state["xyz_max"][i]) - float(state["xyz_min"][i]) for i in range(3)]
        h.S = int(math.sqrt(sum(e * e for e in ext)) * (1 + 1e-5) / h.stepdist) + 2
    if v in ("fourier", "dcvgo"):
        h.t = model_oracle.sample_t(int(state["world_len"]), stepsize, float(state["bg_len"]), t_boundary=2 if v == "dcvgo" else 1.5)
        h.s = 1 - 1 / (1 + h.t)
        h.S = int(h.t.numel())
    if v == "dcvgo":
        h.dist_thres = f32((2 + 2 * float(state["bg_len"])) / int(state["world_len"]) * stepsize * 0.95)
    return h


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def _rel(q, thr):
    """distance of q to its threshold / error unit of q: |q - thr| / max(|q|, thr)"""
    return (q - thr).abs() / q.abs().clamp_min(thr)


def _mask_lookup(state_v, p, dtype):
    """nearest voxel of the mask cache (C round(): half away from zero; outside the grid: False).  Returns the value, the
    distance of the rounding to .5 where a flip along any axes would read another value (inf elsewhere), and the coordinates"""
    mask = state_v["mask"].bool()
    sc = torch.as_tensor(state_v["xyz2ijk_scale"], dtype=torch.float32).to(dtype)
    sh = torch.as_tensor(state_v["xyz2ijk_shift"], dtype=torch.float32).to(dtype)
    c = p * sc + sh
    r = torch.sign(c) * torch.floor(c.abs() + 0.5)
    alt = torch.floor(c) + torch.ceil(c) - r              # the other neighbour (= r for an integer coordinate)
    shape = torch.tensor(mask.shape)

    def read(idx):
        ok = ((idx >= 0) & (idx < shape)).all(-1)
        i = idx.long().clamp_min(0).minimum(shape - 1)
        return mask[i[..., 0], i[..., 1], i[..., 2]] & ok

    val = read(r)
    differ = torch.zeros_like(val)
    for bits in range(1, 8):
        pick = torch.tensor([(bits >> a) & 1 for a in range(3)], dtype=torch.bool)
        differ |= read(torch.where(pick, alt, r)) != val
    frac = c - torch.floor(c)
    dist = (frac - 0.5).abs().amin(-1)
    return val, torch.where(differ, dist, torch.full_like(dist, float("inf"))), c


def _outside(p, lo, hi):
    """mask_outbbox and the distance of p to the nearest box face in units of that axis's extent"""
    out = ((lo > p) | (hi < p)).any(-1)
    d = torch.minimum((p - lo).abs(), (p - hi).abs()) / (hi - lo)
    return out, d.amin(-1)


def _alpha(dens, shift, interval, dtype):
    if dtype == torch.float32:      # the oracle's C restatement of the reference kernel: expf, powf
        return ref_ops.raw2alpha(dens.flatten().contiguous(), shift, interval)[1].reshape(dens.shape)
    return 1 - (1 + torch.exp(dens + shift)) ** (-interval)


@torch.no_grad()
def march_reference(state, rays_o, rays_d, stepsize, dtype, near=0.0):
    """-> namespace of [R, S] tensors: pos [R, S, 3], ran (the ray took the step), evald (density evaluated), dens, alpha, T
    (before the step), w, a_ok (alpha > thres), surv; q = {decision: (quantity or distance [R, S], taken [R, S])}; per ray
    last, depth, wsum_mid (dcvgo), n (dvgo: step count)."""
    h = host_params(state, stepsize, near)
    v, S, R = h.variant, h.S, rays_o.shape[0]
    thres = float(state["fast_color_thres"])
    o, d = rays_o.to(dtype), rays_d.to(dtype)
    lo, hi = state["xyz_min"].to(dtype), state["xyz_max"].to(dtype)
    ones = torch.ones(R, S, dtype=torch.bool)
    q, raws = {}, {}
    n_steps = None
    inner = ones
    if v in ("fourier", "dcvgo"):
        pos, inner = model_oracle.contracted_sample_ray(o, d, state["scene_center"].to(dtype), state["scene_radius"].to(dtype),
                                                        h.t.to(dtype), float(state["bg_len"]), state.get("contracted_norm", "inf"))
        ran, geom = ones, ones
        if v == "dcvgo":
            oo = (o - state["scene_center"].to(dtype)) / state["scene_radius"].to(dtype)
            raw = oo[:, None] + (d / d.norm(dim=-1, keepdim=True))[:, None] * h.t.to(dtype)[None, :, None]
            nrm = raw.abs().amax(-1) if state.get("contracted_norm", "inf") == "inf" else raw.norm(dim=-1)
            q["inner"] = (_rel(nrm, 1.0), ones)
            raws["nrm"] = nrm
            dist = (pos[:, 1:] - pos[:, :-1]).norm(dim=-1)
            cum, over, cums = torch.zeros(R, dtype=dtype), torch.zeros(R, S, dtype=torch.bool), torch.zeros(R, S, dtype=dtype)
            for j in range(1, S):                      # cumdist_thres: a serial recurrence per ray
                cum = cum + dist[:, j - 1]
                cums[:, j] = cum
                over[:, j] = cum > h.dist_thres
                cum = torch.where(over[:, j], torch.zeros_like(cum), cum)
            took = ones.clone()
            took[:, 0] = False
            q["cum"] = (_rel(cums, h.dist_thres), took)
            raws["cum"], raws["over"] = cums, over
            geom = inner | over
    elif v == "dvgo":
        vv = torch.where(d == 0, torch.full_like(d, float(np.float32(1e-6))), d)
        a, b = (hi - o) / vv, (lo - o) / vv
        far = torch.tensor(1e9, dtype=dtype)
        nr = torch.tensor(h.near, dtype=dtype)
        tmin = torch.minimum(torch.minimum(a, b).amax(-1), far).maximum(nr)
        tmax = torch.minimum(torch.maximum(a, b).amin(-1), far).maximum(nr)
        rn = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).sqrt()
        x = (tmax - tmin) * rn / h.stepdist
        n_steps = torch.ceil(x).clamp_min(1).long()
        took = torch.zeros(R, S, dtype=torch.bool)
        took[:, 0] = True
        q["n"] = ((x - torch.round(x).clamp_min(1)).abs()[:, None].expand(R, S), took)
        raws["x"] = x
        j = torch.arange(S)
        ran = j[None, :] < n_steps[:, None]
        dist = h.stepdist * j.to(dtype)
        pos = (o + d * tmin[:, None])[:, None] + (d / rn[:, None])[:, None] * dist[None, :, None]
    else:
        j = torch.arange(S)
        dist = j.to(dtype) / (S - 1)
        pos = o[:, None] + d[:, None] * dist[None, :, None]
        ran = ones
    if v in ("dvgo", "mpi"):
        outside, dface = _outside(pos, lo, hi)
        q["box"] = (dface, ran)
        geom = ran & ~outside
    if v != "fourier":
        mval, mdist, mcoord = _mask_lookup(state[v], pos, dtype)
        q["mask"] = (mdist, geom)
        evald = geom & mval
    else:
        evald, mcoord = geom, None
    F_num = int(state["fourier_freq_num"])
    dens = model_oracle.fourier_grid_query(state["density_grid"].to(dtype), pos, lo, hi, F_num)
    shift = float(np.float32(float(state["act_shift"])))
    if v == "mpi":      # + the per-plane shift, a lerp along z as grid_sample forms it (a corner past the last plane is not added)
        tab = state["mpi"]["act_shift"].reshape(-1).to(dtype)
        D = tab.numel()
        iz = ((((pos[..., 2] - lo[2]) / (hi[2] - lo[2])) * 2 - 1 + 1) / 2) * (D - 1)
        f0 = torch.floor(iz)
        i0 = f0.long().clamp(0, D - 1)
        sh = tab[i0] * ((f0 + 1) - iz)
        dens = dens + torch.where(i0 + 1 <= D - 1, sh + tab[(i0 + 1).clamp(max=D - 1)] * (iz - f0), sh)
    alpha = _alpha(dens, shift, h.interval, dtype)
    # front-to-back compositing: float state, double product, early stop below 1e-3 (Alphas2Weights)
    T = torch.ones(R, dtype=dtype)
    done = torch.zeros(R, dtype=torch.bool)
    out = types.SimpleNamespace(h=h, pos=pos, dens=dens, alpha=alpha, inner=inner, n=n_steps, mcoord=mcoord,
                                T=torch.ones(R, S, dtype=dtype), w=torch.zeros(R, S, dtype=dtype), Tafter=torch.ones(R, S, dtype=dtype),
                                ran=torch.zeros(R, S, dtype=torch.bool), evald=torch.zeros(R, S, dtype=torch.bool),
                                a_ok=torch.zeros(R, S, dtype=torch.bool), surv=torch.zeros(R, S, dtype=torch.bool))
    depth, wmid = torch.zeros(R, dtype=dtype), torch.zeros(R, dtype=dtype)
    for j in range(S):
        live = ~done & ran[:, j]
        ev = live & evald[:, j]
        a_ok = ev & (alpha[:, j] > thres)
        w = T * alpha[:, j]
        Tn = (T.double() * (1.0 - alpha[:, j].double())).to(dtype)
        surv = a_ok & (w > thres)
        out.ran[:, j], out.evald[:, j], out.a_ok[:, j], out.surv[:, j] = live, ev, a_ok, surv
        out.T[:, j], out.w[:, j] = T, torch.where(a_ok, w, torch.zeros_like(w))
        T = torch.where(a_ok, Tn, T)
        out.Tafter[:, j] = T
        done = done | (a_ok & (T.double() < 1e-3))
        if v in ("fourier", "dcvgo"):
            sj = h.s[j].to(dtype)
        elif v == "dvgo":
            sj = torch.tensor(float(j), dtype=dtype)
        else:
            sj = (torch.tensor(float(j), dtype=dtype) + 0.5) / torch.tensor(float(S), dtype=dtype)
        depth = depth + torch.where(surv, w * sj, torch.zeros_like(w))
        wmid = wmid + torch.where(surv & inner[:, j], w, torch.zeros_like(w))
    out.last, out.depth, out.wsum_mid = T, depth, (wmid if v == "dcvgo" else None)
    q = {k: (val, took & out.ran) for k, (val, took) in q.items()}
    q["alpha"] = (_rel(alpha, thres), out.evald)
    q["w"] = (_rel(out.w, thres), out.a_ok)
    q["T"] = (_rel(out.Tafter, 1e-3), out.a_ok)
    out.q, out.raw = q, raws
    return out


def survivors(ref):
    """ray-major survivor list of a reference run, as the oracles return it: ray_id, step_id, weights"""
    idx = ref.surv.nonzero()
    return idx[:, 0], idx[:, 1], ref.w[ref.surv]


# raw (un-normalised) quantities behind each decision, for the float32-vs-float64 error in the decision's own unit
def _decision_errors(r32, r64, state, thres):
    """{decision: largest |q32 - q64| in the decision's unit over the steps at which float64 takes it}"""
    h, v = r64.h, r64.h.variant
    e = {}

    def worst(a32, a64, unit, taken):
        if not bool(taken.any()):
            return 0.0
        return float(((a32.double() - a64) .abs() / unit)[taken].max())

    same = ((r32.surv == r64.surv) & (r32.a_ok == r64.a_ok) & (r32.ran == r64.ran)).all(dim=1)[:, None]       # the same trajectory
    e["alpha"] = worst(r32.alpha, r64.alpha, r64.alpha.abs().clamp_min(thres), r64.evald)
    e["w"] = worst(r32.w, r64.w, r64.w.abs().clamp_min(thres), r64.a_ok & same)
    e["T"] = worst(r32.Tafter, r64.Tafter, r64.Tafter.abs().clamp_min(1e-3), r64.a_ok & same)
    lo, hi = state["xyz_min"].double(), state["xyz_max"].double()
    if v in ("dvgo", "mpi"):
        e["box"] = worst(r32.pos, r64.pos, (hi - lo), r64.q["box"][1][..., None].expand_as(r64.pos))
    if v != "fourier":
        e["mask"] = worst(r32.mcoord, r64.mcoord, 1.0, r64.q["mask"][1][..., None].expand_as(r64.pos))
    if v == "dcvgo":
        e["inner"] = worst(r32.raw["nrm"], r64.raw["nrm"], r64.raw["nrm"].clamp_min(1.0), r64.q["inner"][1])
        same_over = (r32.raw["over"] == r64.raw["over"]).all(dim=1)[:, None]       # (the recurrence restarts at every `over`)
        e["cum"] = worst(r32.raw["cum"], r64.raw["cum"], r64.raw["cum"].clamp_min(h.dist_thres), r64.q["cum"][1] & same_over)
    if v == "dvgo":
        e["n"] = float((r32.raw["x"].double() - r64.raw["x"]).abs().max())
    return e


class Analysis:
    """float64 + float32 runs of a case, its margin, decided steps and e32 of every compared output"""

    def __init__(self, case):
        st = case.state
        self.r64 = r64 = march_reference(st, case.rays_o, case.rays_d, case.stepsize, torch.float64, case.near)
        self.r32 = r32 = march_reference(st, case.rays_o, case.rays_d, case.stepsize, torch.float32, case.near)
        thres = float(st["fast_color_thres"])
        self.e_dec = _decision_errors(r32, r64, st, thres)
        self.m_dec = {k: K * v for k, v in self.e_dec.items()}       # every decision is held to ITS error
        self.m = max(self.m_dec.values())                             # the case's margin: the widest of them
        R, S = r64.ran.shape
        decided = torch.ones(R, S, dtype=torch.bool)
        for k, (val, taken) in r64.q.items():
            exact_tie = (val == 0) & (r32.q[k][0] == 0)
            decided &= ~taken | exact_tie | (val.double() > self.m_dec[k])
        self.decided = decided                                        # [R, S]; steps the ray did not run are decided
        und = ~self.decided & r64.ran
        self.first_undecided = torch.where(und.any(1), und.int().argmax(1), torch.full((R,), S))       # [R]: S = decidable
        self.decidable = self.first_undecided == S
        self.set_aside = 1.0 - float(self.decidable.float().mean())
        # e32 of the outputs, over the decidable rays whose float32 run took the same decisions
        ok = self.decidable & ((r32.surv == r64.surv) & (r32.a_ok == r64.a_ok) & (r32.ran == r64.ran)).all(dim=1)
        self.same32 = ok
        ext = float((st["xyz_max"] - st["xyz_min"]).max())

        def worst(a32, a64, sel):
            return float((a32.double() - a64).abs()[sel].max()) if bool(sel.any()) else 0.0
        sv = r64.surv & ok[:, None]
        self.e32 = {"w": worst(r32.w, r64.w, sv), "last": worst(r32.last, r64.last, ok), "depth": worst(r32.depth, r64.depth, ok),
                    "pos": worst(r32.pos, r64.pos, sv[..., None].expand_as(r64.pos)) / ext}
        if r64.wsum_mid is not None:
            self.e32["wsum_mid"] = worst(r32.wsum_mid, r64.wsum_mid, ok)
        self.pos_floor = 2.0 ** (math.floor(math.log2(ext)) - 23)     # one ulp of the box extent
        self.ext = ext

    def bound(self, key):
        """absolute bound of an output against float64"""
        if key == "pos":
            return K * max(self.e32["pos"] * self.ext, self.pos_floor)
        return K * max(self.e32[key], FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------------------------
def _smooth_noise(g, n_ch, shape, amp):
    x = torch.empty(n_ch, 1, *shape).normal_(0.0, 1.0, generator=g)
    for _ in range(2):
        x = torch.nn.functional.avg_pool3d(x, 5, stride=1, padding=2, count_include_pad=False)
    return x / x.std() * amp


def raw_for_alpha(alpha, interval, shift):
    """the raw density at which alpha = 1 - (1 + exp(raw + shift)) ^ -interval"""
    return math.log((1 - alpha) ** (-1 / interval) - 1) - shift


def density_field(kind, shape, P, interval, shift, seed=0, alpha=0.02, flip_z=False):
    """[P, 1, X, Y, Z]: level 0 carries P x the field (the query takes the mean over the levels), the other levels smooth noise
    where the scene is not meant to be exact.  Coordinates: the grid spans [-1.2, 1.2]^3 whatever the box."""
    g = torch.Generator().manual_seed(seed)
    X, Y, Z = torch.meshgrid(*[torch.linspace(-1.2, 1.2, n) for n in shape], indexing="ij")
    dens = torch.zeros(P, 1, *shape)
    if kind == "empty":
        dens[0, 0] = P * -40.0
    elif kind == "opaque":
        dens[0, 0] = P * 30.0
    elif kind == "capacity":      # alpha ~ 0.02: 0.98^48 = 0.38, so every w stays above 0.005 and no ray reaches T < 1e-3 (mpi: 0.1 over 21
        # steps, 0.9^21 = 0.11 -- at its interval of 11.6 the fp32 rounding of 1 + exp(x) alone is 5e-5 of an alpha of 0.02)
        dens[:, :] = _smooth_noise(g, P, shape, 0.15 * min(1.0, 0.5 / interval))
        dens[0, 0] += P * raw_for_alpha(alpha, interval, shift)
    elif kind == "faint":         # alpha = 0.16 everywhere: T = 0.84^j reaches 1e-3 at step 39 of 42, so a ray's last entries weigh 2e-4, what a
        # composite at 1e-4 hardly sees (an alpha NEAR thres would do that at every step, but 2^-24 is 6e-4 of such an alpha: no margin)
        dens[:, :] = _smooth_noise(g, P, shape, 0.02)
        dens[0, 0] += P * raw_for_alpha(alpha, interval, shift)
    elif kind == "one_lane":      # a solid half space x > 0.1, two-valued
        dens[0, 0] = P * torch.where(X > 0.1, torch.tensor(30.0), torch.tensor(-40.0))
    elif kind == "surfaces":      # the shapes of the trained-like field of tests/test_gpu_march_waves.py: ground slab, lower far shell, spheres.
        # Its densities are chosen for the margin: alpha = 1 - pow(1 + exp(x), -interval) is rounded to 2^-24 in ABSOLUTE terms, 6e-4 of
        # a threshold of 1e-4, so a field with soft transitions (or an empty space of -6: alpha 1e-7 +- 6e-9) always has samples whose
        # alpha decision no fp32 evaluation settles.  Here every voxel is either solid, alpha ~ 0.85 (0.15^k stays clear of 1e-3; rays die after
        # a few samples, at another step each), or EMPTY = -3e6: inside a cell with corners of both kinds the density passes from
        # "alpha is 0 in every precision" to "alpha > 0.01" within 1e-5 of the cell's width, which no sample of these rays hits.
        w = 0.5 * 2.4 / (max(shape) - 1)
        occ = torch.sigmoid((-0.45 - Z) / w)
        if flip_z:                # mpi: every ray crosses the whole depth -- the ground under half of the scene only, no far shell
            occ = occ * (X < 0.2).float()
        cheb = torch.maximum(torch.maximum(X.abs(), Y.abs()), Z.abs())
        # (the far shell by the larger of the two norms, from 1.05: the far samples of either contraction pile up at 1.2, inside it,
        # not in its transition -- there one sample in twenty would sit within the margin of the alpha threshold)
        far = torch.maximum(cheb, (X ** 2 + Y ** 2 + Z ** 2).sqrt())
        if not flip_z:
            occ = torch.maximum(occ, torch.sigmoid((far - 1.05) / w) * (Z < 0.1).float())
        for c, r in (((0.55, 0.45, 0.15), 0.22), ((-0.3, 0.5, 0.0), 0.25), ((0.6, -0.2, 0.3), 0.18), ((0.1, 0.75, 0.45), 0.2)):
            occ = torch.maximum(occ, torch.sigmoid((r - ((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2).sqrt()) / w))
        dens[:, :] = _smooth_noise(g, P, shape, 2.0 * min(1.0, 0.5 / interval))
        dens[0, 0] = P * torch.where(occ > 0.5, torch.tensor(raw_for_alpha(0.85, interval, shift)), torch.tensor(EMPTY))
    else:
        raise KeyError(kind)
    return (dens.flip(-1) if flip_z else dens).contiguous()       # (mpi rays run from z = lo to z = hi: the sky first)


# ---------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------
def fan(R, eye, az0, az1, el0, el1):
    """R rays from `eye`: azimuths x 10 elevations (degrees), elevation fastest, so every 64-ray tile spans all elevations;
    un-normalised directions, like a pinhole camera's"""
    n_el = min(10, R)
    n_az = (R + n_el - 1) // n_el
    az = torch.linspace(math.radians(az0), math.radians(az1), n_az).repeat_interleave(n_el)[:R]
    el = torch.linspace(math.radians(el0), math.radians(el1), n_el).repeat(n_az)[:R]
    d = torch.stack([el.cos() * az.cos(), el.cos() * az.sin(), el.sin()], dim=1) * torch.linspace(0.7, 1.9, R)[:, None]
    return torch.tensor(eye, dtype=torch.float32).expand(R, 3).contiguous(), d.contiguous()


INSIDE = ((0.3, 0.2, 0.4), 0.0, 90.0, -60.0, 40.0)
OUTSIDE = ((1.7, 0.25, 0.3), 150.0, 215.0, -35.0, 25.0)      # eye in the contracted shell, the fan partly through the inner cube
AXIS = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=torch.float32)


def lone_lanes(R):
    """one ray per tile: lane 17, or the last lane of a shorter tile"""
    return [min(t + 17, R - 1) for t in range(0, R, 64)]


def _box(state):
    return state["xyz_min"].float(), state["xyz_max"].float()


def rays_for(variant, kind, R, state):
    """(rays_o, rays_d) of a scene kind, in the variant's world coordinates"""
    lo, hi = _box(state)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    if variant in ("fourier", "dcvgo"):
        c, r = state["scene_center"].float(), state["scene_radius"].float()
        if kind == "one_lane":      # 63 rays of a tile start inside the solid, one starts in the void and looks away from it
            o, d = fan(R, (0.6, 0.2, 0.4), -50.0, 50.0, -40.0, 40.0)
            for i in lone_lanes(R):
                o[i] = torch.tensor([-0.5, 0.1, 0.2])
                d[i] = torch.tensor([-1.3, 0.2, 0.1])
        elif kind == "shell":       # origins outside the unit cube; axis-parallel, un-normalised directions among them
            o, d = fan(R, *OUTSIDE)
            k = min(6, R)
            d[1:1 + k] = AXIS[:k] * 3.0
        else:
            o, d = fan(R, *INSIDE)
        return (o * r + c).contiguous(), d
    if variant == "dvgo":
        # origins inside the box unless stated: a ray that enters through a face puts its first sample ON the face
        if kind == "one_lane":
            o, d = fan(R, (0.55, 0.2, 0.1), -40.0, 40.0, -30.0, 30.0)
            o = mid + o * half * 0.9
            for i in lone_lanes(R):
                o[i] = mid + torch.tensor([-0.5, 0.3, -0.93]) * half
                d[i] = torch.tensor([0.0, 0.0, 1.1])
            return o.contiguous(), d
        o, d = fan(R, (0.1, -0.2, 0.15), 0.0, 350.0, -70.0, 70.0)
        o = mid + o * half
        if kind == "geometry" and R >= 64:
            d[3], d[4], d[5] = torch.tensor([0.0, 0.9, 0.3]), torch.tensor([0.0, 0.0, -1.4]), torch.tensor([1.2, 0.0, 0.0])   # zero components
            for i in range(8, 16):                         # rays that miss the box: origin above it, looking further up
                o[i] = hi + torch.tensor([0.3 + 0.01 * i, 0.2, 0.4])
                d[i] = torch.tensor([0.2, 0.1 * (i - 7), 1.0])
            for i in range(20, 26):                        # origin outside, the box entered before `near`: the first sample lies inside
                d[i] = torch.tensor([0.05 * (i - 22), 0.1, 1.0])
                o[i] = torch.stack([mid[0], mid[1], lo[2] - 0.1]) + 0.0 * d[i]
        return o.contiguous(), d.contiguous()
    # mpi: NDC-like rays from the z = lo plane to the z = hi plane: d_z = the box depth exactly, so the last sample lies on the last plane
    g = torch.Generator().manual_seed(100 + R)
    u = torch.rand(R, 2, generator=g) * 1.6 - 0.8
    o = torch.stack([mid[0] + u[:, 0] * half[0], mid[1] + u[:, 1] * half[1], lo[2].expand(R)], 1)
    d = torch.stack([torch.randn(R, generator=g) * 0.08 * half[0], torch.randn(R, generator=g) * 0.08 * half[1], (hi[2] - lo[2]).expand(R)], 1)
    if kind in ("capacity", "faint"):      # every sample of every ray inside the box
        o[:, :2] = mid[:2] + u * 0.7 * half[:2]
        d[:, :2] = d[:, :2].clamp(-0.15, 0.15) * half[:2] / half[:2]
    if kind == "one_lane":
        o[:, 0] = mid[0] + (0.3 + 0.5 * torch.rand(R, generator=g)) * half[0]
        d[:, 0] = d[:, 0].abs()
        for i in lone_lanes(R):
            o[i, 0], d[i, 0] = mid[0] - 0.5 * half[0], -0.1 * half[0]
    elif kind == "geometry" and R >= 64:
        for i in range(8, 16):                             # rays that leave the box through a side
            d[i, 0] = half[0] * (0.6 + 0.1 * (i - 8))
    return o.contiguous(), d.contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# states (the dict fourier_render.FourierGridRenderer takes) and cases
# ---------------------------------------------------------------------------------------------------------------------
ACT_SHIFT = float(model_oracle.act_shift_from_alpha_init(1e-4))


def _mask(kind, lo, hi):
    """mask cache [6, 8, 10] over the grid's box; 'blocks': free-space blocks in it"""
    mask = torch.ones(MASK_SHAPE, dtype=torch.bool)
    if kind == "blocks":
        g = torch.Generator().manual_seed(SEEDS["mask"])
        mask = torch.rand(3, 4, 5, generator=g).repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2) > 0.3
    scale = (torch.Tensor(list(mask.shape)) - 1) / (hi - lo)
    return {"mask": mask, "xyz2ijk_scale": scale, "xyz2ijk_shift": -lo * scale}


def make_state(variant, kind, F=3, norm="inf", stepsize=0.5):
    """kind: empty | opaque | capacity | faint | one_lane | surfaces | shell (fourier, dcvgo: surfaces seen from outside) | geometry (the bounded
    variants' own: surfaces with a blocked mask cache)"""
    field = {"shell": "surfaces", "geometry": "surfaces"}.get(kind, kind)
    base = {"rgbnet_weights": [], "rgbnet_biases": [], "viewbase_pe": 0, "fast_color_thres": THRES, "contracted_norm": norm}
    if variant == "fourier":
        shape, P = (G_FOURIER,) * 3, 1 + 2 * F
        st = dict(base, scene_center=torch.zeros(3), scene_radius=torch.ones(3), xyz_min=torch.full((3,), -1.2), xyz_max=torch.full((3,), 1.2),
                  bg_len=0.2, fourier_freq_num=F, act_shift=ACT_SHIFT, voxel_size_ratio=1.0, world_len=G_FOURIER)
    else:
        shape, P = GRID, 1
        st = dict(base, fourier_freq_num=0, act_shift=ACT_SHIFT, voxel_size_ratio=1.0, bg_len=0.0, world_len=0,
                  xyz_min=torch.tensor(BOX_LO), xyz_max=torch.tensor(BOX_HI))
        st["scene_center"], st["scene_radius"] = (st["xyz_min"] + st["xyz_max"]) * 0.5, (st["xyz_max"] - st["xyz_min"]) * 0.5
    if variant == "dcvgo":
        blo, bhi = torch.tensor(DCVGO_BOX[0]), torch.tensor(DCVGO_BOX[1])
        st.update(scene_center=(blo + bhi) * 0.5, scene_radius=(bhi - blo) * 0.5, xyz_min=torch.full((3,), -1.2), xyz_max=torch.full((3,), 1.2),
                  bg_len=0.2, world_len=DCVGO_WORLD_LEN)
    if variant == "mpi":
        st["voxel_size_ratio"], st["act_shift"] = 256.0 / GRID[2], 0.0      # (the shift is the per-plane table's)
        st["fast_color_thres"] = stepsize / GRID[2] / 5                     # the forward-facing configurations' rule (tests/mpi_cases.py)
    st["k0_grid"] = torch.zeros(1, 3, *shape)
    h = host_params(dict(st, density_grid=torch.zeros(P, 1, *shape), **({variant: {"voxel_size": DVGO_VOXEL}} if variant != "fourier" else {})),
                    stepsize)
    alpha = 0.16 if kind == "faint" else (0.1 if variant == "mpi" else 0.02)
    st["density_grid"] = density_field(field, shape, P, h.interval, ACT_SHIFT, seed=SEEDS.get(field, 0) + F, alpha=alpha, flip_z=variant == "mpi")
    if variant != "fourier":
        vp = _mask("blocks" if kind in ("geometry", "shell") else "full", st["xyz_min"], st["xyz_max"])
        if variant == "dvgo":
            vp["voxel_size"] = DVGO_VOXEL
        if variant == "mpi":      # a trained-looking per-plane shift; small where the scene is meant to be uniform
            g = torch.Generator().manual_seed(SEEDS["act_shift"])
            amp = 0.005 if kind in ("capacity", "faint") else 1.0
            vp["act_shift"] = ACT_SHIFT + torch.randn(GRID[2], generator=g) * amp
        st[variant] = vp
    return st


class Case:
    def __init__(self, variant, kind, R=200, F=3, norm="inf", stepsize=0.5, near=0.0):
        self.variant, self.kind, self.R, self.F, self.norm, self.stepsize = variant, kind, R, F, norm, stepsize
        self.near = near if variant == "dvgo" else 0.0
        self.state = make_state(variant, kind, F, norm, stepsize)
        self.rays_o, self.rays_d = rays_for(variant, kind, R, self.state)
        self.h = host_params(self.state, stepsize, self.near)
        self.S = self.h.S
        tag = "F%d-%s" % (F, norm) if variant == "fourier" else variant + ("-l2" if norm == "l2" else "")
        self.name = "%s-%s-R%d" % (tag, kind, R) + ("" if stepsize == 0.5 or R == RAY_COUNTS[3] else "-s%g" % stepsize)

    def __repr__(self):
        return self.name


SCENES = ("empty", "opaque", "capacity", "one_lane", "surfaces")
DVGO_NEAR = 0.2


@functools.lru_cache(maxsize=None)
def cases(variant, F=3, norm="inf"):
    """the cases of a variant.  fourier: F = 3 takes every scene (+ shell) and the ray counts, the other F surfaces and capacity"""
    mk = lambda kind, R=200, stepsize=0.5: Case(variant, kind, R, F, norm, stepsize, near=DVGO_NEAR)
    if variant == "fourier" and F != 3:
        return (mk("surfaces"), mk("capacity"))
    own = "shell" if variant in ("fourier", "dcvgo") else "geometry"
    out = [mk(k) for k in SCENES + (own,) + (("faint",) if variant == "fourier" else ())]
    # (37 tiles at stepsize 1.0, half the steps: the interval grows with the stepsize and multiplies every density error)
    out += [mk("surfaces", 5), mk("capacity", 5), mk("surfaces", RAY_COUNTS[2]), mk("surfaces", RAY_COUNTS[3], stepsize=1.0)]
    if variant == "mpi":
        out += [mk("geometry", stepsize=1.0), mk("geometry", stepsize=0.7)]
    if variant == "dcvgo":      # k_march_dcvgo<true>: the l2 contraction
        out += [Case(variant, k, 200, F, "l2", 0.5) for k in ("shell", "capacity")]
    return tuple(out)


def all_cases():
    out = []
    for norm in ("inf", "l2"):
        for F in (3, 1, 2, 4, 5):
            out += list(cases("fourier", F, norm))
    for v in VARIANTS[1:]:
        out += list(cases(v))
    return out


@functools.lru_cache(maxsize=None)
def _analysis(name):
    return Analysis(next(c for c in all_cases() if c.name == name))


def analysis(case):
    """the float64 / float32 references of a case, computed once per process"""
    return _analysis(case.name)
