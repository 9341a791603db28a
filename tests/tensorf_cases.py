"""The TensoRF (vector-matrix grid) cases: inputs regenerated from seeds and the float64 formula, shared by
tests/golden/gen_tensorf_golden.py, tests/test_tensorf.py and tests/test_gpu_tensorf.py.  The fixtures (tests/golden/tensorf_*.npz)
hold what the REFERENCE's TensoRFGrid (FourierGrid/grid.py:90-201) gives for these inputs in float32 and in float64, and the
difference of the two per tensor -- the yardstick of every bound of the GPU tests.

The formula below is written from the definition (no grid_sample): per axis the two vertices and weights of
grid_sample(align_corners=True, zeros padding), planes bilinear, vectors linear, the reference's pairing
xy_plane * z_vec | xz_plane * y_vec | yz_plane * x_vec, then f_vec.  Gradients come from autograd over its indexing."""
import itertools

import numpy as np
import torch

FACTORS = ('xy_plane', 'xz_plane', 'yz_plane', 'x_vec', 'y_vec', 'z_vec')
XYZ_MIN, XYZ_MAX = [-1.0, -0.8, -1.2], [1.1, 0.9, 0.7]
TV_W = (0.7, 1.3, 0.4)                 # wx, wy, wz of the total-variation cases (three different numbers: an axis swap shows)
N_POINTS = (0, 1, 63, 4099)            # empty, one lane, a ragged wave, a ragged last block of 17 blocks
N_STORED = 256                         # forward values the fixtures keep per case (the gradients are kept whole)
BOUND_FACTOR = 4                       # a HIP result lies within 4 x the reference's own fp32-vs-fp64 error of the fp64 value

# every world x (R, Rxy) x C: (5,7,9) has three different sizes (axis swaps), (2,3,2) an axis of two vertices; R != Rxy; C = 3 is no
# multiple of 4
WORLDS = ((5, 7, 9), (2, 3, 2))
COMPS = ((3, 3), (4, 2), (1, 1))
CHANNELS = (1, 3, 12)
KERNEL_CASES = [("w%d%d%d_r%d_%d_c%d" % (*w, r, rxy, c), 100 + i, w, r, rxy, c)
                for i, (w, (r, rxy), c) in enumerate(itertools.product(WORLDS, COMPS, CHANNELS))]
# the backward kernel accumulates by one of three schemes (csrc/ugrid_tensorf.hip, ACC): every gradient in LDS (as doubles) where the
# six factors fit -- all the cases above --, the vectors in LDS and the planes by global atomics where only the vectors fit
# ("path_vlds": component-last layout; the canonical one takes global atomics there), global atomics for everything where not even
# those fit beside the f_vec staging ("path_glob").  Small worlds with many components, so that the axes stay short and the
# reference's own fp32 error stays below 1e-5 of each tensor; the fixture keeps only their yardsticks and forward values.
KERNEL_CASES += [("path_vlds_c1", 201, (9, 7, 5), 64, 64, 1), ("path_vlds_c3", 202, (9, 7, 5), 64, 64, 3),
                 ("path_glob_c1", 203, (9, 7, 5), 400, 400, 1), ("path_glob_c12", 204, (9, 7, 5), 85, 85, 12)]


def shapes(world, R, Rxy, C):
    X, Y, Z = world
    s = {'xy_plane': (1, Rxy, X, Y), 'xz_plane': (1, R, X, Z), 'yz_plane': (1, R, Y, Z), 'x_vec': (1, R, X, 1), 'y_vec': (1, R, Y, 1),
         'z_vec': (1, Rxy, Z, 1)}
    if C > 1:
        s['f_vec'] = (R + R + Rxy, C)
    return s


def case_inputs(case):
    """-> params {name: float32 array}, pts [4099, 3] float32, grad_out [4099] or [4099, C] float32.
    Factors ~ N(0, 0.1) like the reference's initialisation, one entry in sixteen 20 x larger (neighbour differences beyond 1: the
    smooth-L1 clamp of the TV gradient is exercised).  Points: uniform in the box widened by 10 % per side (zero padding), the last
    6 + 8 + 13 of them exactly on the six faces, on the eight corners and on inner vertices."""
    name, seed, world, R, Rxy, C = case
    rs = np.random.RandomState(seed)
    params = {}
    for k, shp in shapes(world, R, Rxy, C).items():
        if k == 'f_vec':
            params[k] = rs.uniform(-0.5, 0.5, shp).astype(np.float32)
        else:
            v = rs.normal(0.0, 0.1, shp)
            v = np.where(rs.uniform(size=shp) < 1 / 16, 20.0 * v, v)
            params[k] = v.astype(np.float32)
    lo, hi = np.array(XYZ_MIN), np.array(XYZ_MAX)
    n = max(N_POINTS)
    pts = lo - 0.1 * (hi - lo) + rs.uniform(size=(n, 3)) * 1.2 * (hi - lo)
    special = []
    for a in range(3):
        for side in (lo, hi):
            p = lo + rs.uniform(size=3) * (hi - lo)
            p[a] = side[a]
            special.append(p)
    for c in itertools.product((0, 1), repeat=3):
        special.append(np.where(np.array(c) == 1, hi, lo))
    for _ in range(13):
        ijk = np.array([rs.randint(0, w) for w in world])
        special.append(lo + ijk / (np.array(world) - 1.0) * (hi - lo))
    pts[n - len(special):] = np.array(special)
    pts = pts.astype(np.float32)
    grad_out = rs.normal(0.0, 1.0, (n, C) if C > 1 else (n,)).astype(np.float32)
    return params, pts, grad_out


# ------------------------------------------------------------------------------------------------------------ the float64 formula
def _axis(x, lo, hi, n):
    """the two vertices of one axis and their weights (0 where the vertex is outside [0, n-1]); indices clamped for the gather"""
    lo, hi = float(np.float32(lo)), float(np.float32(hi))      # (the modules keep the bounds as float32 buffers)
    u = (x - lo) / (hi - lo) * 2 - 1
    ix = (u + 1) / 2 * (n - 1)
    f = torch.floor(ix)
    w1 = ix - f
    w0 = (f + 1) - ix
    i0 = f.long()
    i1 = i0 + 1
    w0 = torch.where((i0 >= 0) & (i0 < n), w0, torch.zeros_like(w0))
    w1 = torch.where((i1 >= 0) & (i1 < n), w1, torch.zeros_like(w1))
    return i0.clamp(0, n - 1), i1.clamp(0, n - 1), w0, w1


def _plane(p, ta, tb):
    q = p[0]
    a0, a1, wa0, wa1 = ta
    b0, b1, wb0, wb1 = tb
    return (q[:, a0, b0] * (wa0 * wb0) + q[:, a0, b1] * (wa0 * wb1) + q[:, a1, b0] * (wa1 * wb0) + q[:, a1, b1] * (wa1 * wb1)).T


def _vec(v, t):
    q = v[0, :, :, 0]
    k0, k1, w0, w1 = t
    return (q[:, k0] * w0 + q[:, k1] * w1).T


def features(params, pts, xyz_min=XYZ_MIN, xyz_max=XYZ_MAX):
    """[n, Rxy + R + R] in the reference's order xy*z | xz*y | yz*x; params: {name: tensor}, any floating type (float64 for the tests)"""
    X, Y = params['xy_plane'].shape[2:]
    Z = params['xz_plane'].shape[3]
    dt = params['xy_plane'].dtype
    pts = pts.to(dt)
    tx = _axis(pts[:, 0], xyz_min[0], xyz_max[0], X)
    ty = _axis(pts[:, 1], xyz_min[1], xyz_max[1], Y)
    tz = _axis(pts[:, 2], xyz_min[2], xyz_max[2], Z)
    return torch.cat([_plane(params['xy_plane'], tx, ty) * _vec(params['z_vec'], tz),
                      _plane(params['xz_plane'], tx, tz) * _vec(params['y_vec'], ty),
                      _plane(params['yz_plane'], ty, tz) * _vec(params['x_vec'], tx)], -1)


def query(params, pts, xyz_min=XYZ_MIN, xyz_max=XYZ_MAX):
    """TensoRFGrid.forward: [n] (no f_vec) or [n, C]"""
    feat = features(params, pts, xyz_min, xyz_max)
    return feat @ params['f_vec'] if 'f_vec' in params else feat.sum(-1)


def dense(params):
    """TensoRFGrid.get_dense_grid: [1, C, X, Y, Z]"""
    xy, xz, yz = params['xy_plane'][0], params['xz_plane'][0], params['yz_plane'][0]
    xv, yv, zv = params['x_vec'][0, :, :, 0], params['y_vec'][0, :, :, 0], params['z_vec'][0, :, :, 0]
    feat = torch.cat([xy[:, :, :, None] * zv[:, None, None, :], xz[:, :, None, :] * yv[:, None, :, None],
                      yz[:, None, :, :] * xv[:, :, None, None]])
    if 'f_vec' in params:
        return torch.einsum('rxyz,rc->cxyz', feat, params['f_vec'])[None]
    return feat.sum(0)[None, None]


def trilinear(grid, pts, xyz_min=XYZ_MIN, xyz_max=XYZ_MAX):
    """zero-padded trilinear lookup of a dense [1, C, X, Y, Z] grid: [n, C]"""
    _, C, X, Y, Z = grid.shape
    pts = pts.to(grid.dtype)
    tx = _axis(pts[:, 0], xyz_min[0], xyz_max[0], X)
    ty = _axis(pts[:, 1], xyz_min[1], xyz_max[1], Y)
    tz = _axis(pts[:, 2], xyz_min[2], xyz_max[2], Z)
    out = 0
    for a, b, c in itertools.product((0, 1), repeat=3):
        out = out + grid[0][:, tx[a], ty[b], tz[c]] * (tx[2 + a] * ty[2 + b] * tz[2 + c])
    return out.T


def _smooth_l1_sum(a, b):
    d = a - b
    return torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).sum()


def tv_loss(params, wx, wy, wz):
    """the loss of TensoRFGrid.total_variation_add_grad (grid.py:142-154)"""
    p = params
    s = _smooth_l1_sum
    loss = wx * s(p['xy_plane'][:, :, 1:], p['xy_plane'][:, :, :-1]) + wy * s(p['xy_plane'][:, :, :, 1:], p['xy_plane'][:, :, :, :-1]) \
        + wx * s(p['xz_plane'][:, :, 1:], p['xz_plane'][:, :, :-1]) + wz * s(p['xz_plane'][:, :, :, 1:], p['xz_plane'][:, :, :, :-1]) \
        + wy * s(p['yz_plane'][:, :, 1:], p['yz_plane'][:, :, :-1]) + wz * s(p['yz_plane'][:, :, :, 1:], p['yz_plane'][:, :, :, :-1]) \
        + wx * s(p['x_vec'][:, :, 1:], p['x_vec'][:, :, :-1]) + wy * s(p['y_vec'][:, :, 1:], p['y_vec'][:, :, :-1]) \
        + wz * s(p['z_vec'][:, :, 1:], p['z_vec'][:, :, :-1])
    return loss / 6


def as_f64(params):
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in params.items()}


def reference_f64(case, n):
    """float64 values of one case on its first n points by the formula above: {'out', 'dense', 'g_<name>', 'tv_<name>'} (numpy)"""
    params, pts, grad_out = case_inputs(case)
    p = {k: v.requires_grad_(True) for k, v in as_f64(params).items()}
    pts_t, g = torch.from_numpy(pts[:n]), torch.from_numpy(grad_out[:n]).double()
    out = query(p, pts_t)
    res = {'out': out.detach().numpy(), 'dense': dense(p).detach().numpy()}
    names = list(p)
    grads = torch.autograd.grad((out * g).sum(), [p[k] for k in names], allow_unused=True) if n > 0 else [None] * len(names)
    for k, gr in zip(names, grads):
        res['g_' + k] = (torch.zeros_like(p[k]) if gr is None else gr).numpy()
    tv = torch.autograd.grad(tv_loss(p, *TV_W), [p[k] for k in FACTORS], allow_unused=True)
    for k, gr in zip(FACTORS, tv):
        res['tv_' + k] = (torch.zeros_like(p[k]) if gr is None else gr).numpy()
    return res


def load_yardsticks(golden_dir):
    """{case name: {'n<k>/<tensor>': (err, scale)}} from tests/golden/tensorf_kernels.npz"""
    import os
    z = np.load(os.path.join(golden_dir, "tensorf_kernels.npz"))
    out = {}
    for key in z.files:
        if key.endswith("/yard"):
            case, rest = key[:-5].split("/", 1)
            out.setdefault(case, {})[rest] = tuple(float(x) for x in z[key])
    return out


# ------------------------------------------------------------------------------------------------------------ whole models
# name, kind, density grid, seed of the model's initialisation, seed of the rays
MODEL_CASES = [("dvgo_tt", "dvgo", "TensoRFGrid", 5, 6), ("dcvgo_tt", "dcvgo", "TensoRFGrid", 7, 8), ("dvgo_dt", "dvgo", "DenseGrid", 9, 10)]
MODEL_KEYS = ("weights", "raw_alpha", "raw_rgb", "rgb_marched", "alphainv_last")
RENDER_KW = dict(near=0.2, far=6.0, stepsize=0.5, bg=1)
TRAIN_STEPS, TRAIN_SEED, TRAIN_RAY_SEED, TRAIN_VOXELS = 40, 21, 22, 16 ** 3
TRAIN_CFG = dict(lrate_density=0.1, lrate_k0=0.1, lrate_rgbnet=3e-3, lrate_decay=20, pg_scale=[20], decay_after_scale=1.0, weight_main=1.0,
                 weight_entropy_last=0.01, weight_rgbper=0.01, weight_nearclip=0.0, weight_distortion=0.0, tv_every=1, tv_after=0,
                 tv_before=20, tv_dense_before=10, weight_tv_density=1e-5, weight_tv_k0=1e-6, skip_zero_grad_fields=['density', 'k0'])


def model_kwargs(kind, density_type, width=32, nvox=12 ** 3):
    """12^3 voxels, n_comp 3 (density) and 5 (k0), rgbnet width 32"""
    kw = dict(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=nvox, num_voxels_base=nvox, alpha_init=1e-2, fast_color_thres=1e-4,
              density_type=density_type, density_config=dict(n_comp=3) if density_type == 'TensoRFGrid' else {}, k0_type='TensoRFGrid',
              k0_config=dict(n_comp=5), rgbnet_dim=12, rgbnet_width=width)
    if kind == 'dvgo':
        kw['rgbnet_direct'] = True
    return kw


def model_rays(n, seed, kind='dvgo'):
    """origins on a sphere around the box [-1, 1]^3 (radius 3; the contracted model: 0.6, inside the separating cube), each looking
    at a point inside it -> rays_o, rays_d, viewdirs [n, 3] float32"""
    rs = np.random.RandomState(seed)
    o = rs.normal(size=(n, 3))
    o = 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rs.uniform(-0.8, 0.8, (n, 3)) - o
    v = d / np.linalg.norm(d, axis=1, keepdims=True)
    if kind == 'dcvgo':
        o = o * 0.2
    return [a.astype(np.float32) for a in (o, d, v)]


def structure_density(model, density_type):
    """a density field with structure instead of the initial near-zero one: TensoRF factors x 12, dense voxels ~ N(0, 3) from a seed"""
    with torch.no_grad():
        if density_type == 'TensoRFGrid':
            for p in model.density.parameters():
                p.mul_(12.0)
        else:
            g = torch.Generator().manual_seed(3)
            model.density.grid.copy_(torch.randn(model.density.grid.shape, generator=g) * 3.0)


def train_target(viewdirs):
    return (0.5 + 0.4 * torch.sin(3.0 * viewdirs + torch.tensor([0.0, 1.0, 2.0], dtype=viewdirs.dtype, device=viewdirs.device))).contiguous()
