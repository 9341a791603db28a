"""The march at 7 and 8 waves per SIMD (k_march_ring, ug_density_ring: the level sum as a hand-pipelined ring of brick loads behind counted vmcnt
waits, csrc/ugrid_render.h) against the 6-wave kernel (plain C++ loads).  Only the order of issue differs, so every output must be
bit-identical: alphainv_last, depth, rgb_marched and the survivor count, for every instantiation F = 1..5 x both contractions, on a
field where the ring is always full (white noise, few rays terminate) and on one where lanes go `done` in the middle of a tile
(surfaces: exec-masked loads inside the ring), plus a camera outside the unit cube (part of a tile's samples in the contracted shell
before the tile enters the inner volume).

Shapes: G = 24, C = 12, the rgbnet of the benchmark (39-128-128-3), 200 rays = three full 64-ray tiles + one partial tile of 8,
stepsize 0.85 -> 48 samples a ray."""
import math

import pytest
import torch

G, C, PE, R, STEPSIZE = 24, 12, 4, 200, 0.85
DENS_MEAN, DENS_STD = -8.5, 24.0       # the benchmark's white-noise density statistics
WAVES = (6, 7, 8)


def _rgbnet(g):
    dims = [C + 3 + 6 * PE, 128, 128, 3]
    ws, bs = [], []
    for i in range(3):
        b = 1.0 / math.sqrt(dims[i])
        ws.append(torch.empty(dims[i + 1], dims[i]).uniform_(-b, b, generator=g))
        bs.append(torch.empty(dims[i + 1]).uniform_(-b, b, generator=g))
    bs[2].zero_()
    return ws, bs


def _state(dens, k0, ws, bs, F, norm):
    return {
        "density_grid": dens, "k0_grid": k0, "rgbnet_weights": ws, "rgbnet_biases": bs,
        "scene_center": torch.zeros(3), "scene_radius": torch.ones(3),
        "xyz_min": torch.Tensor([-1, -1, -1]) - 0.2, "xyz_max": torch.Tensor([1, 1, 1]) + 0.2,
        "bg_len": 0.2, "fourier_freq_num": F, "viewbase_pe": PE,
        "act_shift": float(torch.FloatTensor([math.log(1 / (1 - 1e-4) - 1)])), "voxel_size_ratio": 1.0,
        "fast_color_thres": 1e-4, "contracted_norm": norm, "world_len": G,
    }


def noise_state(F, norm):
    """white noise: alpha is either ~0 or ~1 per cell, few rays reach T < 1e-3 within 48 samples"""
    g = torch.Generator().manual_seed(11 + F)
    P = 1 + 2 * F
    dens = torch.empty(P, 1, G, G, G).normal_(DENS_MEAN, DENS_STD, generator=g)
    k0 = torch.empty(P, C, G, G, G).normal_(0.0, 1.0, generator=g)
    ws, bs = _rgbnet(g)
    return _state(dens, k0, ws, bs, F, norm)


def surfaces_state(F, norm):
    """trained-like field at G = 24: a ground slab, the lower half of the far shell and a few soft spheres carried by level 0 (raw density
    -6 in empty space, +16 in solids, 1.5-voxel transitions), smooth noise on the other levels: rays that look down end on a surface
    after a few samples, rays that look up leave through empty sky"""
    g = torch.Generator().manual_seed(1000 + F)
    P = 1 + 2 * F
    lin = torch.linspace(-1.2, 1.2, G)
    X, Y, Z = torch.meshgrid(lin, lin, lin, indexing="ij")
    w = 1.5 * 2.4 / (G - 1)
    occ = torch.sigmoid((-0.45 - Z) / w)
    cheb = torch.maximum(torch.maximum(X.abs(), Y.abs()), Z.abs())
    occ = torch.maximum(occ, torch.sigmoid((cheb - 1.12) / w) * (Z < 0.1).float())
    for c, r in (((0.55, 0.45, 0.15), 0.22), ((-0.3, 0.5, 0.0), 0.25), ((0.6, -0.2, 0.3), 0.18), ((0.1, 0.75, 0.45), 0.2)):
        occ = torch.maximum(occ, torch.sigmoid((r - ((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2).sqrt()) / w))

    def smooth_noise(n_ch, amp):
        x = torch.empty(n_ch, 1, G, G, G).normal_(0.0, 1.0, generator=g)
        for _ in range(2):
            x = torch.nn.functional.avg_pool3d(x, 5, stride=1, padding=2, count_include_pad=False)
        return x / x.std() * amp

    dens = smooth_noise(P, 2.0).reshape(P, 1, G, G, G)
    dens[0, 0] = P * (-6.0 + 22.0 * occ)
    k0 = torch.cat([smooth_noise(C, 1.0)[:, 0][None] for _ in range(P)])
    ws, bs = _rgbnet(g)
    return _state(dens.contiguous(), k0, ws, bs, F, norm)


def fan_rays(eye, az0, az1, el0, el1):
    """200 rays from `eye`: 20 azimuths x 10 elevations (degrees), elevation fastest, so every 64-ray tile spans all elevations"""
    az = torch.linspace(math.radians(az0), math.radians(az1), 20).repeat_interleave(10)
    el = torch.linspace(math.radians(el0), math.radians(el1), 10).repeat(20)
    d = torch.stack([el.cos() * az.cos(), el.cos() * az.sin(), el.sin()], dim=1)
    d = d * torch.linspace(0.7, 1.9, R)[:, None]          # un-normalised directions, like a pinhole camera's
    o = torch.tensor(eye).expand(R, 3).contiguous()
    return o, d.contiguous(), (d / d.norm(dim=1, keepdim=True)).contiguous()


INSIDE = ((0.3, 0.2, 0.4), 0.0, 90.0, -60.0, 40.0)        # the benchmark camera's eye, looking over the scene: down to the ground, up to the sky
OUTSIDE = ((1.7, 0.25, 0.3), 150.0, 215.0, -35.0, 25.0)   # eye in the contracted shell, the fan partly through the inner cube, partly past it


@pytest.fixture
def march_waves():
    from unboundednerfpytorch_amd.fourier_render import tune
    yield lambda w: tune("march_waves", w)
    tune("march_waves", 0)          # 0 = the library's default


def render_at_all_waves(state, rays, set_waves):
    from unboundednerfpytorch_amd.fourier_render import FourierGridRenderer
    rend = FourierGridRenderer(state, "cuda:0", pipeline=0)
    o, d, v = [x.cuda() for x in rays]
    res = {}
    for w in WAVES:
        set_waves(w)
        out = rend(o, d, v, stepsize=STEPSIZE, render_depth=True)
        torch.cuda.synchronize()
        res[w] = ({k: out[k].clone() for k in ("alphainv_last", "depth", "rgb_marched")}, rend.survivors_of_last_chunk())
        assert out["n_max"] == 48
    return res


def assert_identical(res):
    ref, m_ref = res[6]
    assert m_ref > 0 and all(bool(torch.isfinite(ref[k]).all()) for k in ref)
    for w in WAVES[1:]:
        out, m = res[w]
        assert m == m_ref, "march_waves %d: %d survivors, %d at 6 waves" % (w, m, m_ref)
        for k in ("alphainv_last", "depth", "rgb_marched"):
            assert torch.equal(out[k], ref[k]), "march_waves %d: %s differs from the 6-wave kernel's (max |d| %g)" % (
                w, k, float((out[k] - ref[k]).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["inf", "l2"])
@pytest.mark.parametrize("F", [1, 2, 3, 4, 5])
def test_ring_full_white_noise(F, norm, march_waves):
    res = render_at_all_waves(noise_state(F, norm), fan_rays(*INSIDE), march_waves)
    assert_identical(res)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["inf", "l2"])
@pytest.mark.parametrize("F", [1, 2, 3, 4, 5])
def test_lanes_done_mid_tile_surfaces(F, norm, march_waves):
    res = render_at_all_waves(surfaces_state(F, norm), fan_rays(*INSIDE), march_waves)
    last = res[6][0]["alphainv_last"]
    for t in range(0, R - 63, 64):  # the case is about (full) tiles in which some rays have terminated and others march on
        done = last[t:t + 64] < 1e-3
        assert bool(done.any()) and not bool(done.all()), "tile %d: %d of %d rays terminated" % (t // 64, int(done.sum()), done.numel())
    assert_identical(res)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["inf", "l2"])
def test_tile_partly_in_the_contracted_shell(norm, march_waves):
    state = surfaces_state(3, norm)
    rays = fan_rays(*OUTSIDE)
    from unboundednerfpytorch_amd.fourier_render import sample_table
    t, _ = sample_table(G, STEPSIZE, 0.2)
    p = rays[0][:, None, :] + rays[2][:, None, :] * t[None, :, None]
    nrm = p.norm(dim=-1) if norm == "l2" else p.abs().amax(dim=-1)
    inner = nrm <= 1.0                                             # [R, S]: sample in the uncontracted volume
    for t0 in range(0, R, 64):      # at the same sample index some rays of the tile are in the shell and others inside
        mixed = inner[t0:t0 + 64].any(dim=0) & ~inner[t0:t0 + 64].all(dim=0)
        assert int(mixed.sum()) >= 4, "tile %d: %d mixed sample indices" % (t0 // 64, int(mixed.sum()))
    assert_identical(render_at_all_waves(state, rays, march_waves))


def test_march_waves_knob_range():
    """host only: the knob takes 4..8 (and 0 = the default), nothing else"""
    from unboundednerfpytorch_amd import _lib
    L = _lib.load()
    try:
        for v in (3, 9, -1, 16):
            assert L.ugrid_tune(b"march_waves", v) != 0, v
        for v in (4, 5, 6, 7, 8):
            assert L.ugrid_tune(b"march_waves", v) == 0, v
    finally:
        assert L.ugrid_tune(b"march_waves", 0) == 0
