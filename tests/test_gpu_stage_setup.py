"""The stage set-up on fused kernels: train_rays.voxel_count_views on ugrid_count_views_accumulate / _commit (the coarse stage's
per-voxel learning rate, dvgo.py:250-276) and train_rays.hit_coarse_geo on ugrid_hit_coarse_geo (the fine stage's ray filter,
dvgo.py:291-304, 619-657), against the composed paths they replace (train_rays.FUSED_SETUP = False: the lookup's autograd backward on
materialised points; sample_pts_on_rays + maskcache_lookup) and the goldens of the reference's own methods
(tests/golden/dvgo_utils.npz).  The counts are the same sums in another order -- exact where every term is dyadic, within the
existing bound of tests/test_gpu_voxgo_train.py::test_dvgo_voxel_count_views_matches_the_reference otherwise --; the hit mask is
bit for bit the composed one."""
import os

import numpy as np
import pytest
import torch

import synth
from test_gpu_voxgo_train import build, DVGO_CASES

MASK_SEED, MASK_DENSITY = 71, 0.05      # chosen on the CPU with the oracle's ops (oracle.ref_ops through train_rays.hit_coarse_geo): 50 % of the views' rays hit


@pytest.fixture
def setup_switch():
    from unboundednerfpytorch_amd import train_rays
    assert train_rays.FUSED_SETUP is True
    yield train_rays
    train_rays.FUSED_SETUP = True


def _both(train_rays, fn):
    """fn() on the fused kernels and on the composed path; the fused entry points are counted to make sure which one ran"""
    from unboundednerfpytorch_amd import _lib
    L = _lib.load()
    names = ("ugrid_count_views_accumulate", "ugrid_count_views_commit", "ugrid_hit_coarse_geo")
    calls = {n: 0 for n in names}
    real = {n: getattr(L, n) for n in names}

    def counted(n):
        def call(*a):
            calls[n] += 1
            return real[n](*a)
        return call
    res = []
    try:
        for n in names:
            setattr(L, n, counted(n))
        for fused in (True, False):
            train_rays.FUSED_SETUP = fused
            before = sum(calls.values())
            res.append(fn())
            assert (sum(calls.values()) > before) == fused, (fused, calls)
    finally:
        for n in names:
            setattr(L, n, real[n])
        train_rays.FUSED_SETUP = True
    return res[0], res[1], calls


def _views(dev):
    from unboundednerfpytorch_amd.fourier_render import get_rays_of_a_view
    H, W, K, poses = synth.dvgo_views()
    ro, rd = [], []
    for c2w in poses:
        o, d, _ = get_rays_of_a_view(H, W, torch.from_numpy(K).to(dev), torch.from_numpy(c2w).to(dev), inverse_y=False, flip_x=False,
                                     flip_y=False)
        ro.append(o.reshape(H, W, 3))
        rd.append(d.reshape(H, W, 3))
    return H, W, K, poses, ro, rd


@pytest.mark.gpu
def test_view_counts_are_exact_where_every_weight_is_dyadic(setup_switch):
    """Box [0,8]^3 with 9^3 vertices (voxel size 1), stepsize 0.5, rays along +z from z = -2 at dyadic (x, y): every coordinate and
    every trilinear weight is a small dyadic number, every sum exact in any order.  Four images of two rays each:
      0: (2,3), (5,5)       -> the full columns (2,3) and (5,5) gather 2.0 (1.5 at the end vertices)
      1: (2.5,3), (6.25,6)  -> column (2,3) gathers exactly 1.0: NOT counted (strict >); (6,6) gathers 1.5, (7,6) 0.5
      2: (2.5,3), (3.5,3)   -> column (3,3) gathers 2.0 from the two half-offset rays; (2,3) and (4,3) exactly 1.0
      3: (20,3), (30,3)     -> miss the box
    The end vertex k = 8 also receives the sample half a cell OUTSIDE the box (z = 8.5, zero padding): a ray must not stop at the face.
    Expected: count = 1 on the four z-columns (2,3), (5,5), (3,3), (6,6), 0 elsewhere: 36 in all."""
    from unboundednerfpytorch_amd import grid as _grid
    train_rays = setup_switch
    dev = torch.device("cuda", 0)
    xy = [(2, 3), (5, 5), (2.5, 3), (6.25, 6), (2.5, 3), (3.5, 3), (20, 3), (30, 3)]
    o = torch.tensor([[x, y, -2.0] for x, y in xy], device=dev)
    d = torch.tensor([[0.0, 0.0, 1.0]] * len(xy), device=dev)
    lo, hi = torch.zeros(3, device=dev), torch.full((3,), 8.0, device=dev)
    want = torch.zeros(1, 1, 9, 9, 9, device=dev)
    for i, j in ((2, 3), (5, 5), (3, 3), (6, 6)):
        want[0, 0, i, j, :] = 1
    assert float(want.sum()) == 36

    def run():
        return train_rays.voxel_count_views(_grid.GridQuery.apply, lo, hi, torch.tensor(1.0, device=dev), torch.tensor([9, 9, 9]), (1, 1, 9, 9, 9),
                                            o, d, [2, 2, 2, 2], 0.2, 0.5, irregular_shape=True)
    fused, composed, calls = _both(train_rays, run)
    assert calls["ugrid_count_views_accumulate"] == 4 and calls["ugrid_count_views_commit"] == 4      # two launches per image
    assert fused.shape == want.shape and fused.dtype == torch.float32
    assert torch.equal(fused, want), (fused - want).nonzero().tolist()
    assert torch.equal(composed, want), (composed - want).nonzero().tolist()
    direct = train_rays.voxel_count_views_fused(lo, hi, torch.tensor(1.0, device=dev), torch.tensor([9, 9, 9]), (1, 1, 9, 9, 9), o, d,
                                                [2, 2, 2, 2], 0.2, 0.5, irregular_shape=True)
    assert torch.equal(direct, want)


@pytest.mark.gpu
def test_fused_view_counts_match_the_composed_ones_and_the_reference(setup_switch, golden_dir):
    """the three views of tests/golden/dvgo_utils.npz on the model of DVGO_CASES[0]: fused vs composed and each vs the reference's
    own count, under the bound the existing test uses for "the same sums in another order" (a voxel whose sum sits within rounding of
    1 may flip); then the two other image selections: downrate = 2 on the image-shaped table, and the imsz split of a flat one"""
    train_rays = setup_switch
    dev = torch.device("cuda", 0)
    m = build("dvgo", DVGO_CASES[0], dev)[0]
    gold = np.load(os.path.join(golden_dir, "dvgo_utils.npz"))
    H, W, K, poses, ro, rd = _views(dev)
    o_tr, d_tr = torch.stack(ro), torch.stack(rd)

    def differ(a, b):
        assert a.shape == b.shape
        return float((a != b).mean())
    kw = dict(near=0.2, far=6.0, stepsize=0.5)
    fused, composed, calls = _both(train_rays, lambda: m.voxel_count_views(rays_o_tr=o_tr, rays_d_tr=d_tr, imsz=1, downrate=1,
                                                                          irregular_shape=False, **kw).cpu().numpy())
    assert calls["ugrid_count_views_accumulate"] == 3 and calls["ugrid_count_views_commit"] == 3
    assert fused.shape == gold["count"].shape and fused.max() >= 2
    assert differ(fused, composed) <= 1e-3
    assert differ(fused, gold["count"]) <= 1e-3 and differ(composed, gold["count"]) <= 1e-3
    fused2, composed2, _ = _both(train_rays, lambda: m.voxel_count_views(rays_o_tr=o_tr, rays_d_tr=d_tr, imsz=1, downrate=2,
                                                                         irregular_shape=False, **kw).cpu().numpy())
    assert differ(fused2, composed2) <= 1e-3 and 0 < fused2.sum() <= fused.sum()
    sizes = [H * W, H * W - 5, H * W + 5]            # the flat table cut into three "images" of unequal size
    fused3, composed3, _ = _both(train_rays, lambda: m.voxel_count_views(rays_o_tr=o_tr.reshape(-1, 3), rays_d_tr=d_tr.reshape(-1, 3), imsz=sizes,
                                                                         downrate=1, irregular_shape=True, **kw).cpu().numpy())
    assert differ(fused3, composed3) <= 1e-3 and fused3.sum() > 0


def _random_mask(m):
    shape = tuple(m.mask_cache.mask.shape)
    mask = torch.from_numpy(synth.uniform(MASK_SEED, int(np.prod(shape))) < MASK_DENSITY).reshape(shape)
    with torch.no_grad():
        m.mask_cache.mask.copy_(mask.to(m.mask_cache.mask.device))


@pytest.mark.gpu
def test_fused_hit_filter_equals_the_composed_one_bit_for_bit(setup_switch, golden_dir):
    """ugrid_hit_coarse_geo against sample_pts_on_rays + maskcache_lookup: the three views plus seven hand-built rays (two that
    miss the box, one starting inside it, two with zero direction components, one running along a face, one pointing away) on a
    seeded random mask cache that between 20 % and 80 % of the rays hit; and, with the model's own mask, against the reference's
    result under the existing bound"""
    train_rays = setup_switch
    dev = torch.device("cuda", 0)
    m = build("dvgo", DVGO_CASES[0], dev)[0]
    gold = np.load(os.path.join(golden_dir, "dvgo_utils.npz"))
    H, W, K, poses, ro, rd = _views(dev)
    kw = dict(near=0.2, far=6.0, stepsize=0.5)
    own_f, own_c, calls = _both(train_rays, lambda: torch.stack([m.hit_coarse_geo(rays_o=o, rays_d=d, **kw) for o, d in zip(ro, rd)]))
    assert calls["ugrid_hit_coarse_geo"] == 3 and own_f.dtype == torch.bool and own_f.shape == (3, H, W)
    assert torch.equal(own_f, own_c)
    assert float((own_f.cpu().numpy() != gold["hit"]).mean()) <= 2e-3
    hand_o = torch.tensor([[-3.0, 2.5, 0.3], [0.2, 0.1, 4.0],           # miss the box (DVGO_BOX: [-1,-0.8,-1.1] .. [1,0.9,1])
                           [0.1, -0.2, 0.3],                            # origin inside
                           [-2.5, 0.1, 0.2], [0.3, -2.0, -0.4],         # zero direction components (one, two)
                           [-3.0, 0.9, 0.2],                            # along the face y = y_max
                           [2.5, 0.0, 0.0]], device=dev)                # pointing away
    hand_d = torch.tensor([[0.5, 0.1, -0.05], [0.3, 0.2, 0.4], [0.4, -0.3, 0.2], [1.0, 0.0, 0.1], [0.0, 1.5, 0.0], [1.0, 0.0, 0.0],
                           [1.0, 0.1, 0.1]], device=dev)
    o = torch.cat([x.reshape(-1, 3) for x in ro] + [hand_o])
    d = torch.cat([x.reshape(-1, 3) for x in rd] + [hand_d])
    _random_mask(m)
    fused, composed, _ = _both(train_rays, lambda: m.hit_coarse_geo(rays_o=o, rays_d=d, **kw))
    assert fused.shape == (3 * H * W + 7,) and fused.dtype == torch.bool
    share = float(fused.float().mean())
    assert 0.2 <= share <= 0.8, share
    assert torch.equal(fused, composed), (fused != composed).nonzero().flatten().tolist()
    assert fused[-7:-5].tolist() == [False, False] and fused[-1:].tolist() == [False]
    # the same on a full mask: every ray that has a sample inside the box hits -- the walk's box test alone
    with torch.no_grad():
        m.mask_cache.mask.fill_(True)
    fused, composed, _ = _both(train_rays, lambda: m.hit_coarse_geo(rays_o=o, rays_d=d, **kw))
    assert torch.equal(fused, composed) and fused[-7:].tolist() == [False, False, True, True, True, True, False]


@pytest.mark.gpu
def test_in_maskcache_ray_table_is_the_same_with_the_fused_filter(setup_switch):
    """get_training_rays_in_maskcache_sampling (dvgo.py:619-657) end to end: all five outputs equal with the filter fused or composed"""
    from unboundednerfpytorch_amd.dvgo_render import get_training_rays_in_maskcache_sampling
    train_rays = setup_switch
    dev = torch.device("cuda", 0)
    m = build("dvgo", DVGO_CASES[0], dev)[0]
    _random_mask(m)
    H, W, K, poses = synth.dvgo_views()
    imgs = [torch.from_numpy(synth.uniform(900 + i, H * W * 3).reshape(H, W, 3)).to(dev) for i in range(len(poses))]
    rk = dict(near=0.2, far=6.0, stepsize=0.5)
    fused, composed, calls = _both(train_rays, lambda: get_training_rays_in_maskcache_sampling(
        imgs, [torch.from_numpy(p) for p in poses], [(H, W)] * len(poses), [K] * len(poses), False, False, False, False, m, rk))
    assert calls["ugrid_hit_coarse_geo"] == len(poses)
    assert len(fused) == len(composed) == 5
    for a, b in zip(fused[:4], composed[:4]):
        assert a.shape == b.shape and torch.equal(a, b)
    assert [int(x) for x in fused[4]] == [int(x) for x in composed[4]]
    assert 0.2 * 3 * H * W <= fused[0].shape[0] <= 0.8 * 3 * H * W
