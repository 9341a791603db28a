"""Hand-built work lists for the shade half of the fused render (ugrid_render_shade: k_shade_mlp, k_shade_pc, k_shade_direct)
and its plain reference.  TEST INFRASTRUCTURE: tests/test_shade_cases.py (CPU) checks this file, tests/test_gpu_shade_worklist.py
runs the kernels on what it builds.

The shade stage has no thresholds: it is a continuous function of (work list, view directions, k0 grid, rgbnet), so it is held
to a bound far below the rendered frames' 1e-4, with no ray set aside, against the SAME formula evaluated in float64:

    features  = model_oracle.fourier_grid_query(k0 grid, entry positions)          (mean over levels of trilinear taps)
    net input = [features | viewdir_embedding(v)[ray]]
    logits    = rgbnet_apply(...)        (+ k0[:, :3], the net fed k0[:, 3:], for residual colour; = the features without an rgbnet)
    rgb[ray]  = sum over the ray's entries, in list order, of w * sigmoid(logits)

The work list is the byte layout of csrc/ugrid_render.h: ug_ws_make -- 256 B of tile counters | count [n_tiles] int32 |
ent [n_tiles][64 S] float4 (world x, y, z, weight) | slot [n_tiles][64 S] uint8, every region aligned to 256 B -- written
here directly, so a test chooses the shapes a march of a random scene never produces on demand: a tile filled to capacity, a pass
of 32 survivors owned by one ray, counts of 15 / 16 / 17 ... around the pass and half-pass sizes, a lone survivor in slot 63, a
last tile of 37 rays, more tiles than persistent waves.

The bound.  e32 = max |shade_reference(float32) - shade_reference(float64)| is the reference's OWN fp32 error on a case; the kernel
must stay within K * max(e32, 2^-23) of the float64 result on every ray.  K = 8 for the fp32 and bf16x3 rgbnet arithmetics (products
at 2^-24 per include/ugrid_hip.h): the kernel differs from the oracle's fp32 evaluation in three places, each worth about one e32 --
the brick polynomial instead of the 8-tap interpolation, device sin / cos within 2 ulp, the MFMA summation order -- and a maximum
over a few thousand samples fluctuates by about 2 x.  K = 32 for fp16x2, whose products are 2^-22, four times coarser.  The CPU suite
asserts e32 <= 3e-7 for every case, so no bound exceeds 1e-5."""
import ctypes
import functools

import numpy as np
import torch

import synth
from oracle import model_oracle

# the (F, C, PE) triples of UG_SHADE_TRIPLES (csrc/ugrid_shade.hip); tests/test_shade_cases.py compares with the source
TRIPLES = ((3, 12, 4), (4, 12, 4), (5, 12, 4), (2, 12, 4), (1, 12, 4), (0, 12, 4), (2, 3, 2), (3, 3, 2), (3, 12, 8), (3, 3, 8),
           (3, 15, 4), (3, 9, 4), (0, 9, 4), (0, 9, 0))
RESIDUAL_TRIPLES = ((0, 12, 4), (0, 9, 4), (3, 12, 4))
PROBE_TRIPLES = ((3, 12, 4), (2, 3, 2), (3, 15, 4), (3, 9, 4), (3, 12, 8))
MLP_FP32, MLP_BF16X3, MLP_FP16X2 = 0, 1, 2
MODE_NAME = {0: "fp32", 1: "bf16x3", 2: "fp16x2"}

GRID = (7, 9, 11)                                   # X, Y, Z: small, non-cubic
BOX_LO, BOX_HI = (-1.0, -0.5, -2.0), (1.0, 1.5, 1.0)  # off the origin, another extent per axis
S_SMALL, N_RAYS = 4, 613                            # capacity 256 entries per tile; 10 tiles, 37 rays in the last one
SENTINEL, GUARD_ROWS = -7.25, 64
K_BOUND = {MLP_FP32: 8.0, MLP_BF16X3: 8.0, MLP_FP16X2: 32.0}
K_DIRECT = 8.0                                      # the no-rgbnet kernel: plain fp32
E32_LIMIT = 3e-7
FLOOR = 2.0 ** -23


def modes_of(F, C, pe):
    """the rgbnet arithmetics ugrid_render_shade accepts for a tabulated triple (ug_shade_launch, csrc/ugrid_shade.hip): fp16x2
    keeps a per-wave embedding table in LDS that does not fit for viewbase_pe = 8; the exact-fp32 variant of C = 9 with an
    embedding is not built"""
    if pe > 4:
        return (MLP_FP32, MLP_BF16X3)
    if C == 9 and pe != 0:
        return (MLP_BF16X3, MLP_FP16X2)
    return (MLP_FP32, MLP_BF16X3, MLP_FP16X2)


# ---------------------------------------------------------------------------------------------------------------------
# work list bytes
# ---------------------------------------------------------------------------------------------------------------------
def _a256(x):
    return (x + 255) & ~255


def worklist_regions(n_rays, S):
    """n_tiles, capacity per tile, byte offsets of count / ent / slot, total bytes"""
    nt, cap = (n_rays + 63) // 64, 64 * S
    off_count = 256
    off_ent = off_count + _a256(nt * 4)
    off_slot = off_ent + _a256(nt * cap * 16)
    return nt, cap, off_count, off_ent, off_slot, off_slot + _a256(nt * cap)


def rays_in_tile(n_rays, t):
    return min(64, n_rays - 64 * t)


def write_worklist(n_rays, S, tiles, poison=False):
    """tiles: one (ent [n, 4] float32 = world x, y, z, weight; slot [n] uint8 = ray slot inside the tile) per 64-ray tile, in list
    order -> the work list as a torch.uint8 tensor of ugrid_render_ws_bytes(n_rays, S) bytes (the caller asserts the size).
    Beyond a tile's count: zeros, or with poison=True NaN positions and weights and the slot of a ray of that tile that owns no
    entry -- a kernel that reads past the count shows a NaN in a ray whose colour must be exactly 0, and cannot index out of range."""
    nt, cap, oc, oe, os_, total = worklist_regions(n_rays, S)
    assert len(tiles) == nt, (len(tiles), nt)
    buf = np.zeros(total, dtype=np.uint8)
    count = buf[oc:oc + nt * 4].view(np.int32)
    ent = buf[oe:oe + nt * cap * 16].view(np.float32).reshape(nt, cap, 4)
    slot = buf[os_:os_ + nt * cap].reshape(nt, cap)
    for t, (e, s) in enumerate(tiles):
        e, s = np.asarray(e, dtype=np.float32).reshape(-1, 4), np.asarray(s, dtype=np.uint8).reshape(-1)
        n, live = s.shape[0], rays_in_tile(n_rays, t)
        assert e.shape[0] == n and n <= cap, (t, n, cap)
        assert n == 0 or int(s.max()) < live, (t, int(s.max()), live)       # a slot beyond the tile's rays names no ray
        count[t] = n
        ent[t, :n] = e
        slot[t, :n] = s
        if poison and n < cap:
            free = np.setdiff1d(np.arange(live), s)
            assert free.size > 0, "tile %d: poison needs a ray without entries" % t
            ent[t, n:] = np.nan
            slot[t, n:] = free[-1]
    return torch.from_numpy(buf)


def read_worklist(ws, n_rays, S):
    """inverse of write_worklist on a host copy of a work list: [(ent [n, 4], slot [n])] per tile"""
    nt, cap, oc, oe, os_, total = worklist_regions(n_rays, S)
    buf = ws.detach().cpu().contiguous().numpy()
    assert buf.dtype == np.uint8 and buf.shape[0] >= total
    count = buf[oc:oc + nt * 4].view(np.int32)
    ent = buf[oe:oe + nt * cap * 16].view(np.float32).reshape(nt, cap, 4)
    slot = buf[os_:os_ + nt * cap].reshape(nt, cap)
    assert int(count.min()) >= 0 and int(count.max()) <= cap
    return [(ent[t, :count[t]].copy(), slot[t, :count[t]].copy()) for t in range(nt)]


def flatten(tiles):
    """list order -> pos [M, 3], w [M] (float32 tensors) and ray_id [M] (int64)"""
    if sum(len(s) for _, s in tiles) == 0:
        return torch.zeros(0, 3), torch.zeros(0), torch.zeros(0, dtype=torch.int64)
    ent = np.concatenate([np.asarray(e, dtype=np.float32).reshape(-1, 4) for e, _ in tiles])
    rid = np.concatenate([64 * t + np.asarray(s, dtype=np.int64) for t, (_, s) in enumerate(tiles)])
    return torch.from_numpy(ent[:, :3].copy()), torch.from_numpy(ent[:, 3].copy()), torch.from_numpy(rid)


class WorkList:
    """a list + its rays' view directions; `same`: groups of rays that own the same entry sequence and view direction"""

    def __init__(self, name, n_rays, S, tiles, viewdirs, same=()):
        self.name, self.n_rays, self.S, self.tiles, self.viewdirs, self.same = name, n_rays, S, tiles, viewdirs, same
        self.pos, self.w, self.ray_id = flatten(tiles)
        self.counts = [len(s) for _, s in tiles]
        self.empty_rays = torch.ones(n_rays, dtype=torch.bool)
        self.empty_rays[self.ray_id] = False

    def bytes(self, poison=False):
        return write_worklist(self.n_rays, self.S, self.tiles, poison=poison)


# ---------------------------------------------------------------------------------------------------------------------
# entries: positions, weights, view directions
# ---------------------------------------------------------------------------------------------------------------------
_LO, _HI = np.array(BOX_LO, dtype=np.float32), np.array(BOX_HI, dtype=np.float32)


def box_features():
    """the 26 corner / edge-midpoint / face-centre points of the box"""
    mid = (_LO + _HI) * np.float32(0.5)
    pts = [[(_LO, mid, _HI)[k][ax] for ax, k in enumerate((i, j, l))] for i in range(3) for j in range(3) for l in range(3)
           if (i, j, l) != (1, 1, 1)]
    return np.array(pts, dtype=np.float32)


def positions(rng, n, grid=GRID):
    """n points of the box, a quarter each: uniform | corners, edges, faces | exact grid vertices lo + i ext / (n - 1) | cell centres"""
    ext, g1 = _HI - _LO, np.array(grid, dtype=np.float32) - np.float32(1)
    out = (_LO + ext * rng.rand(n, 3).astype(np.float32)).astype(np.float32)
    kind = (np.arange(n) + rng.randint(4)) % 4
    feats = box_features()
    out[kind == 1] = feats[rng.randint(len(feats), size=int((kind == 1).sum()))]
    iv = np.stack([rng.randint(0, g, size=n) for g in grid], 1).astype(np.float32)            # 0 .. n-1: the last vertex included
    ic = np.stack([rng.randint(0, g - 1, size=n) for g in grid], 1).astype(np.float32)
    out[kind == 2] = (_LO + iv * ext / g1)[kind == 2]
    out[kind == 3] = (_LO + (ic + np.float32(0.5)) * ext / g1)[kind == 3]
    return np.clip(out, _LO, _HI).astype(np.float32)      # (fp32 rounding of lo + (n-1) ext / (n-1) may pass hi by an ulp)


def weights(rng, slot):
    """random weights whose per-ray sums stay below 1 (what front-to-back compositing produces), with exact zeros and 1e-12 among them"""
    slot = np.asarray(slot)
    w = rng.rand(slot.shape[0]) + 1e-3
    for r in np.unique(slot):
        m = slot == r
        w[m] *= rng.uniform(0.3, 0.999) / w[m].sum()
    w = w.astype(np.float32)
    if w.shape[0] >= 8:
        w[rng.randint(w.shape[0])] = 0.0
        w[rng.randint(w.shape[0])] = 1e-12
    return w


def make_tile(rng, slot):
    slot = np.asarray(slot, dtype=np.uint8)
    return np.concatenate([positions(rng, slot.shape[0]), weights(rng, slot)[:, None]], 1).astype(np.float32), slot


def unit_viewdirs(rng, n):
    v = rng.randn(n, 3)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


AXIS_DIRS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
SEQ_LEN = 40        # the shared entry sequence: longer than a pass


def _with_sequence(rng, count, seq, owner, other_slots, force=()):
    """a tile of `count` entries: `seq` (ent [n, 4]) in order, owned by slot `owner`, at random places among entries of other rays
    (the first of which belong to the slots `force`)"""
    n = seq.shape[0]
    where = np.sort(rng.choice(count, size=n, replace=False))
    slot = rng.choice(other_slots, size=count).astype(np.uint8)
    slot[where] = owner
    rest = np.setdiff1d(np.arange(count), where)
    slot[rest[:len(force)]] = force
    ent, _ = make_tile(rng, slot)
    ent[where] = seq
    return ent, slot


@functools.lru_cache(maxsize=None)
def lists():
    """name -> WorkList.  'a' and 'b' (613 rays, S = 4) hold every tile kind between them; 'five' is one tile of five rays; 'many'
    (S = 1) has 256 * 8 + 11 tiles, more than the persistent shade kernels have waves, so that waves take a second tile and rebuild
    their embedding table, and every ray owns at most ONE entry, so rgb = w * sigmoid(logit) with no per-ray sum behind it (the column
    probe's list); 'empty' has no entry at all."""
    rng = np.random.RandomState(20241)
    out = {}
    seq_slot = np.zeros(SEQ_LEN, dtype=np.uint8)
    seq = make_tile(rng, seq_slot)[0]

    def counted(n, force=()):
        slot = rng.choice(np.arange(0, 63), size=n)
        slot[:len(force)] = force
        return make_tile(rng, slot)

    # ---- list a
    t0 = _with_sequence(rng, 97, seq, 0, np.arange(1, 63), force=(1, 2, 3, 4, 5, 6))      # the six axis-direction rays own entries
    full = _with_sequence(rng, 64 * S_SMALL, seq, 63, np.arange(0, 63))
    owners = [5, 63, 5, 0, 17]                               # every pass of 32 belongs to one ray; the last pass is partial
    one_ray = make_tile(rng, np.concatenate([np.full(32 if i < 4 else 9, o) for i, o in enumerate(owners)]))
    alternating = make_tile(rng, np.tile([10, 11], 35))
    last_a = _with_sequence(rng, 75, seq, 36, np.setdiff1d(np.arange(0, 36), [20]))
    tiles_a = [t0, make_tile(rng, []), make_tile(rng, [63]), counted(15), counted(16), counted(17), full, one_ray, alternating, last_a]
    va = unit_viewdirs(rng, N_RAYS)
    va[1:7] = AXIS_DIRS
    ray_a, ray_b, ray_c = 0, 6 * 64 + 63, 9 * 64 + 36
    va[ray_b] = va[ray_c] = va[ray_a]
    out["a"] = WorkList("a", N_RAYS, S_SMALL, tiles_a, torch.from_numpy(va), same=((ray_a, ray_b, ray_c),))
    # ---- list b
    # march-like: step-major, lanes ascending, random survival (lane 40 never survives: poison needs a ray without entries)
    march = np.concatenate([np.nonzero((rng.rand(64) < 0.6) & (np.arange(64) != 40))[0] for _ in range(S_SMALL)])
    last_b = make_tile(rng, rng.choice(np.setdiff1d(np.arange(0, 37), [36]), size=50))
    tiles_b = [make_tile(rng, march), counted(31, force=(1, 2, 3, 4, 5, 6)), counted(32), counted(33), counted(47), counted(48), counted(49),
               make_tile(rng, []), make_tile(rng, rng.choice(np.arange(0, 64), size=64 * S_SMALL)), last_b]
    vb = unit_viewdirs(rng, N_RAYS)
    vb[64 + 1:64 + 7] = AXIS_DIRS
    out["b"] = WorkList("b", N_RAYS, S_SMALL, tiles_b, torch.from_numpy(vb))
    # ---- one tile of five rays
    out["five"] = WorkList("five", 5, S_SMALL, [make_tile(rng, rng.choice(np.arange(0, 4), size=11))], torch.from_numpy(unit_viewdirs(rng, 5)))
    # ---- more tiles than persistent waves, about two entries each
    nt = 256 * 8 + 11
    n_many = 64 * (nt - 1) + 40
    many = []
    for t in range(nt):
        live = rays_in_tile(n_many, t)
        many.append(make_tile(rng, rng.choice(np.arange(0, live - 1), size=rng.randint(0, 5), replace=False)))
    vm = unit_viewdirs(rng, n_many)
    owners_m = np.concatenate([64 * t + s_.astype(np.int64) for t, (_, s_) in enumerate(many)])
    vm[owners_m[:6]] = AXIS_DIRS                   # (every ray of this list owns at most one entry)
    out["many"] = WorkList("many", n_many, 1, many, torch.from_numpy(vm))
    out["empty"] = WorkList("empty", N_RAYS, S_SMALL, [make_tile(rng, []) for _ in range(10)], torch.from_numpy(unit_viewdirs(rng, N_RAYS)))
    return out


MAIN_LISTS = ("a", "b")


# ---------------------------------------------------------------------------------------------------------------------
# scenes: k0 grid + rgbnet
# ---------------------------------------------------------------------------------------------------------------------
class Scene:
    """kg [P, C, X, Y, Z] float32; nets = ([w0, w1, w2], [b0, b1, b2]) in nn.Linear layout, or None (rgb = sigmoid(k0), C = 3, F = 0).
    residual: the net reads [k0[3:], embedding] (w0 has C - 3 + 3 + 6 pe columns) and k0[:3] is added to its logits."""

    def __init__(self, F, C, pe, kg, nets, residual=False, lo=BOX_LO, hi=BOX_HI):
        self.F, self.C, self.pe, self.kg, self.nets, self.residual = F, C, pe, kg, nets, bool(residual)
        self.lo, self.hi = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
        self.grid = tuple(int(x) for x in kg.shape[2:])
        self.mlp_in = 0 if nets is None else C + 3 + 6 * pe


def random_nets(seed, n_in, width=128):
    dims = [n_in, width, width, 3]
    ws, bs = [], []
    for li in range(3):
        b = 1.0 / np.sqrt(dims[li])
        ws.append(torch.from_numpy(synth.uniform(seed + 10 + li, dims[li + 1] * dims[li], -b, b).reshape(dims[li + 1], dims[li])))
        bs.append(torch.from_numpy(synth.uniform(seed + 20 + li, dims[li + 1], -b, b)))
    return ws, bs


@functools.lru_cache(maxsize=None)
def scene(F, C, pe, residual=False, rgbnet=True, wide_k=0, grid=GRID):
    """deterministic scene of a triple; wide_k: k0 x 10^k with the first layer x 10^-k (operands far from 1, the same order of logits)"""
    seed = 9000 + 100 * F + 7 * C + pe + (50 if residual else 0)
    if not rgbnet:
        assert F == 0 and C == 3
        kg = torch.from_numpy(synth.normal(seed, 3 * int(np.prod(grid)), 0.0, 1.0).reshape(1, 3, *grid))
        return Scene(0, 3, pe, kg, None)
    P = 1 + 2 * F
    kg = torch.from_numpy(synth.normal(seed, P * C * int(np.prod(grid)), 0.0, 1.0).reshape(P, C, *grid))
    ws, bs = random_nets(seed, (C - 3 if residual else C) + 3 + 6 * pe)
    if wide_k:
        kg = kg * float(10 ** wide_k)
        ws = [ws[0] * float(10 ** -wide_k)] + ws[1:]
    return Scene(F, C, pe, kg, (ws, bs), residual=residual)


def probe_nets(mlp_in, cols):
    """a net that routes three input columns unchanged to the three logits: unit 2j = relu(+x_c), unit 2j+1 = relu(-x_c), identity
    second layer, last layer +1 / -1 -- every product is by 0 or 1, so rgb = w * sigmoid(column) isolates the gather and the embedding"""
    w0, w1, w2 = torch.zeros(128, mlp_in), torch.eye(128), torch.zeros(3, 128)
    for j, c in enumerate(cols):
        w0[2 * j, c], w0[2 * j + 1, c] = 1.0, -1.0
        w2[j, 2 * j], w2[j, 2 * j + 1] = 1.0, -1.0
    return [w0, w1, w2], [torch.zeros(128), torch.zeros(128), torch.zeros(3)]


def probe_column_sets(mlp_in):
    cols = list(range(mlp_in)) + [0, 1][:(-mlp_in) % 3]
    return [tuple(cols[i:i + 3]) for i in range(0, len(cols), 3)]


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def shade_inputs(sc, wl, dtype):
    """[M, C] k0 features and [M, 3 + 6 pe] view embedding of the list's entries, evaluated in `dtype`"""
    k0 = model_oracle.fourier_grid_query(sc.kg.to(dtype), wl.pos.to(dtype), sc.lo.to(dtype), sc.hi.to(dtype), sc.F)
    emb = model_oracle.viewdir_embedding(wl.viewdirs.to(dtype), sc.pe)[wl.ray_id]
    return k0.reshape(wl.pos.shape[0], sc.C), emb


@torch.no_grad()
def shade_reference(sc, wl, dtype, nets=None):
    """rgb_marched [n_rays, 3] of the work list in `dtype` (float32: the oracle's arithmetic; float64: the truth).  nets: another
    rgbnet than the scene's (the column probe)."""
    out = torch.zeros(wl.n_rays, 3, dtype=dtype)
    if wl.pos.shape[0] == 0:
        return out
    k0, emb = shade_inputs(sc, wl, dtype)
    nets = sc.nets if nets is None else nets
    if nets is None:
        logits = k0
    else:
        ws, bs = [w.to(dtype) for w in nets[0]], [b.to(dtype) for b in nets[1]]
        if sc.residual:
            logits = model_oracle.rgbnet_apply(ws, bs, torch.cat([k0[:, 3:], emb], -1)) + k0[:, :3]
        else:
            logits = model_oracle.rgbnet_apply(ws, bs, torch.cat([k0, emb], -1))
    return out.index_add_(0, wl.ray_id, wl.w.to(dtype).unsqueeze(-1) * torch.sigmoid(logits))      # (CPU index_add_: in list order)


_REFS = {}


def references(sc, wl):
    """(ref64 [n_rays, 3] float64, e32) of a (scene, list) pair, computed once"""
    key = (id(sc), wl.name)
    if key not in _REFS:
        r64 = shade_reference(sc, wl, torch.float64)
        e32 = float((shade_reference(sc, wl, torch.float32).double() - r64).abs().max()) if wl.pos.shape[0] else 0.0
        _REFS[key] = (sc, r64, e32)      # (the scene is kept alive: its id is the key)
    return _REFS[key][1:]


def wide_range_k():
    """the largest k <= 3 at which the wide-range scene (k0 x 10^k, first layer x 10^-k) still has e32 <= E32_LIMIT on the main lists"""
    for k in (3, 2, 1):
        sc = scene(3, 12, 4, wide_k=k)
        if all(references(sc, lists()[n])[1] <= E32_LIMIT for n in MAIN_LISTS):
            return k
    raise AssertionError("no wide-range scene meets the fp32 condition")


def all_scenes():
    """(tag, scene) of every case of the GPU file that is held to the bound"""
    out = [("F%d-C%d-pe%d" % t, scene(*t)) for t in TRIPLES]
    out += [("F%d-C%d-pe%d-residual" % t, scene(*t, residual=True)) for t in RESIDUAL_TRIPLES]
    out += [("no-rgbnet", scene(0, 3, 0, rgbnet=False)), ("wide-k%d" % wide_range_k(), scene(3, 12, 4, wide_k=wide_range_k()))]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the device side: pack + one ugrid_render_shade call (no renderer objects: the F = 0 triples would need mask caches)
# ---------------------------------------------------------------------------------------------------------------------
class Packed:
    """k0 bricks + packed rgbnet of a scene on the device, filled the way FourierGridRenderer.__init__ fills them"""

    def __init__(self, sc, nets=None, device="cuda:0"):
        from unboundednerfpytorch_amd import _lib
        self._lib, self.L, self.sc, self.dev = _lib, _lib.load(), sc, torch.device(device)
        L, p = self.L, _lib.ptr
        st = torch.cuda.current_stream(self.dev).cuda_stream
        kg = sc.kg.to(self.dev, torch.float32).contiguous()
        P, C = int(kg.shape[0]), sc.C
        X, Y, Z = sc.grid
        nets = sc.nets if nets is None else nets
        direct = 1 if nets is None else 0
        self.k0_bricks = torch.empty(L.ugrid_brick_bytes(P, C, X, Y, Z, direct) // 4, dtype=torch.float32, device=self.dev)
        _lib.check(L.ugrid_pack_bricks(p(kg), P, C, X, Y, Z, direct, p(self.k0_bricks), st), "pack k0")
        self.mlp_packed, self.best_mode = None, None
        if nets is not None:
            ws, bs = [w.clone() for w in nets[0]], nets[1]
            if sc.residual:      # zero columns for the three diffuse channels: the matrix chain ignores them, the epilogue adds them
                ws[0] = torch.cat([ws[0].new_zeros(ws[0].shape[0], 3), ws[0]], dim=1)
            assert ws[0].shape == (128, sc.mlp_in) and ws[1].shape == (128, 128) and ws[2].shape == (3, 128)
            t = [x.to(self.dev, torch.float32).contiguous() for x in (ws[0], bs[0], ws[1], bs[1], ws[2], bs[2])]
            self.mlp_packed = torch.empty(L.ugrid_mlp_packed_bytes(C, sc.pe) // 4, dtype=torch.float32, device=self.dev)
            best = ctypes.c_int32(-1)
            _lib.check(L.ugrid_pack_mlp(*[p(x) for x in t], C, sc.pe, 128, float(kg.abs().max()), p(self.mlp_packed),
                                        ctypes.byref(best), st), "pack mlp")
            self.best_mode = int(best.value)
        torch.cuda.current_stream(self.dev).synchronize()

    def params(self, n_rays, S, mlp_mode, **override):
        sc, q = self.sc, self._lib.RenderParams()
        q.n_rays, q.n_samples, q.freq_num = n_rays, S, sc.F
        q.grid_x, q.grid_y, q.grid_z = sc.grid
        q.k0_channels, q.mlp_in, q.mlp_width = sc.C, sc.mlp_in, 128
        q.viewbase_pe, q.norm_l2 = sc.pe, 0
        for i in range(3):
            q.scene_center[i], q.scene_radius[i] = 0.0, 1.0
            q.xyz_min[i], q.xyz_max[i] = float(sc.lo[i]), float(sc.hi[i])
        q.bg_len, q.act_shift, q.interval, q.thres = 0.2, 0.0, 0.5, 1e-4
        q.mlp_mode = int(mlp_mode) | (self._lib.MLP_RESIDUAL if sc.residual else 0)
        for k, v in override.items():
            setattr(q, k, v)
        return q

    def shade(self, ws_dev, viewdirs_dev, n_rays, S, mlp_mode=0, **override):
        """one ugrid_render_shade call -> (its return value, rgb [n_rays + GUARD_ROWS, 3] pre-filled with SENTINEL) after a sync"""
        p = self._lib.ptr
        rgb = torch.full((n_rays + GUARD_ROWS, 3), SENTINEL, dtype=torch.float32, device=self.dev)
        q = self.params(n_rays, S, mlp_mode, **override)
        st = torch.cuda.current_stream(self.dev).cuda_stream
        err = self.L.ugrid_render_shade(q, p(viewdirs_dev), p(self.k0_bricks), p(self.mlp_packed), p(ws_dev), p(rgb), st)
        torch.cuda.synchronize(self.dev)
        return int(err), rgb.cpu()


def pack(kg, nets, C, pe, residual, F=None, lo=BOX_LO, hi=BOX_HI, device="cuda:0"):
    """k0 grid [P, C, X, Y, Z] + 128-wide nets (or None) -> Packed, through ugrid_pack_bricks / ugrid_pack_mlp (k0_absmax = max |kg|)"""
    F = (int(kg.shape[0]) - 1) // 2 if F is None else F
    return Packed(Scene(F, C, pe, kg, nets, residual=residual, lo=lo, hi=hi), device=device)
