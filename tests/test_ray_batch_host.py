"""train_rays.RayBatcher on the CPU (the torch composition of `batch`, which shares its index logic -- view search, local pixel,
restricted rows -- with ugrid_ray_batch), device_batch_indices_generator and sample_batch_lazy against the goldens of the
reference's own functions (tests/golden/train_rays.npz, rebuilt inputs: gen_train_rays_golden.scene) -- bitwise, the criterion
tests/test_train_rays.py applies to the table path on the CPU.  No GPU needed."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
GOLD = os.path.join(ROOT, "tests", "golden", "train_rays.npz")
FLAGS = dict(ndc=False, inverse_y=True, flip_x=False, flip_y=True)


def scene():
    import gen_train_rays_golden as gen
    return gen.scene()


def same(a, b):
    np.testing.assert_array_equal(a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a), b)


def test_all_rows_in_order_equal_the_reference_tables():
    from unboundednerfpytorch_amd import train_rays as tr
    g = np.load(GOLD)
    imgs, poses, HW, Ks = scene()
    total = sum(int(h) * int(w) for h, w in HW)
    every = torch.arange(total)
    b = tr.RayBatcher.from_views(imgs, poses.clone(), HW, Ks, with_index=True, **FLAGS)
    assert len(b) == total and b.device.type == "cpu"
    out = b.batch(every)
    for k, v in zip(("rgb", "o", "d", "v", "idx"), out):
        assert v.dtype == torch.float32 and v.shape == (total, 3)
        same(v, g["fg_" + k])
    assert list(b.imsz) == list(g["fg_imsz"])
    b = tr.RayBatcher.from_views(imgs, poses.clone(), HW, Ks, with_index=False, **FLAGS)
    out = b.batch(every)
    for k, v in zip(("rgb", "o", "d", "v"), out[:4]):
        same(v, g["flat_" + k])
    assert out[4] is None and list(b.imsz) == list(g["flat_imsz"])
    p2 = poses.clone()
    b = tr.RayBatcher.from_views(imgs, p2, HW, Ks, with_index=True, pos_emb=torch.tensor([0.1, -0.2, 0.05]), **FLAGS)
    same(b.batch(every)[1], g["fgpos_o"])
    same(p2, g["fgpos_poses_after"])                  # refined in place, like the reference
    # nothing of the table's size beyond the images: the float store is the images, flattened
    assert b.resident_bytes() == total * 12 + 96 * 3 + 8 * 4
    # a permuted, repeating index list gives the same rows as indexing the table
    sel = torch.from_numpy(np.random.RandomState(0).randint(0, total, 97))
    for v, k in zip(b.batch(sel)[2:5], ("d", "v", "idx")):
        same(v, g["fg_" + k][sel.numpy()])


def test_index_and_table_sizes_are_validated_on_the_host():
    from unboundednerfpytorch_amd import train_rays as tr
    imgs, poses, HW, Ks = scene()
    b = tr.RayBatcher.from_views(imgs, poses.clone(), HW, Ks, with_index=False, **FLAGS)
    with pytest.raises(ValueError):
        b.batch(torch.arange(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        b.batch(torch.arange(4).reshape(2, 2))
    with pytest.raises(ValueError):
        tr.RayBatcher.from_views(imgs[:2], poses.clone(), HW, Ks, with_index=False, **FLAGS)
    with pytest.raises(ValueError):
        tr.RayBatcher.from_views(imgs, poses.clone(), HW[[1, 0, 2]], Ks, with_index=False, **FLAGS)   # another view's size
    with pytest.raises(ValueError):
        tr.RayBatcher.from_views(imgs, poses.clone(), HW, Ks, with_index=False, store="float16", **FLAGS)
    out = b.batch(torch.zeros(0, dtype=torch.int64))
    assert [tuple(t.shape) for t in out[:4]] == [(0, 3)] * 4


def test_device_sampler_follows_the_numpy_stream():
    from unboundednerfpytorch_amd import train_rays as tr
    g = np.load(GOLD)
    np.random.seed(11)
    gen = tr.device_batch_indices_generator(50, 16, "cpu")
    got = [next(gen) for _ in range(7)]
    assert all(t.dtype == torch.int64 and t.device.type == "cpu" for t in got)
    same(torch.stack(got), g["sampler_batches"])
    # three epochs of N = 50, BS = 16: tail drop (2 of 50) and redraw, batch for batch the host generator under the same seed
    np.random.seed(4)
    ref = tr.batch_indices_generator(50, 16)
    ref = [next(ref) for _ in range(9)]
    np.random.seed(4)
    gen = tr.device_batch_indices_generator(50, 16, "cpu")
    for want in ref:
        assert torch.equal(next(gen), want)
    assert len(set(torch.cat(ref[:3]).tolist())) == 48 and not torch.equal(ref[0], ref[3])


def test_random_mode_makes_the_draws_of_sample_batch():
    from unboundednerfpytorch_amd import train_rays as tr
    g = np.load(GOLD)
    imgs, poses, HW, Ks = scene()
    shaped = tr.RayBatcher.from_views(torch.stack([imgs[0], imgs[2]]), poses[[0, 2]], HW[[0, 2]], np.stack([Ks[0], Ks[0]]), ndc=False,
                                      inverse_y=False, flip_x=True, flip_y=False, with_index=False, image_shaped=True)
    flat = tr.RayBatcher.from_views(imgs, poses.clone(), HW, Ks, with_index=False, **FLAGS)
    assert shaped.image_shape == (2, 6, 9) and shaped.imsz == [1, 1] and flat.image_shape is None
    cfg = {"ray_sampler": "random", "N_rand": 10}
    torch.manual_seed(5)
    t, o, d, v, idx = tr.sample_batch_lazy(cfg, shaped, None)
    same(t, g["rand3_target"])
    same(o, g["rand3_o"])
    assert idx is None
    t, *_ = tr.sample_batch_lazy(cfg, flat, None)
    same(t, g["rand2_target"])
    same(torch.rand(3), g["rand_next"])               # same number of draws as run_train.py
    with pytest.raises(NotImplementedError):
        tr.sample_batch_lazy({"ray_sampler": "spiral", "N_rand": 10}, flat, None)


def test_lazy_gather_dispatches_like_gather_training_rays():
    from unboundednerfpytorch_amd import train_rays as tr
    g = np.load(GOLD)
    imgs, poses, HW, Ks = scene()
    cfg = types.SimpleNamespace(model="FourierGrid", data=types.SimpleNamespace(
        dataset_type="tankstemple", load2gpu_on_the_fly=True, ndc=False, inverse_y=True, flip_x=False, flip_y=True))
    cfg_train = types.SimpleNamespace(ray_sampler="flatten", N_rand=32)
    args = ({"irregular_shape": True}, imgs, cfg, [0, 1, 2], cfg_train, poses, HW, Ks, {})
    np.random.seed(2)
    table = tr.gather_training_rays(types.SimpleNamespace(pos_emb=None), *args, device="cpu")
    ref = [tr.sample_batch(cfg_train, *table[:5], table[6], device="cpu", load2gpu_on_the_fly=True) for _ in range(6)]
    np.random.seed(2)
    batcher, imsz, sampler = tr.gather_training_rays_lazy(types.SimpleNamespace(pos_emb=None), *args, device="cpu")
    assert batcher.with_index and list(imsz) == list(g["fg_imsz"]) == list(table[5])
    for want in ref:
        got = tr.sample_batch_lazy(cfg_train, batcher, sampler)
        assert len(got) == 5 and all(torch.equal(a, b) for a, b in zip(got, want))
    cfg.model = "DVGO"                                # non-FourierGrid models follow cfg_train.ray_sampler
    batcher, imsz, _ = tr.gather_training_rays_lazy(types.SimpleNamespace(), *args, device="cpu")
    assert not batcher.with_index and batcher.image_shape is None and list(imsz) == list(g["flat_imsz"])
    cfg_train.ray_sampler = "random"                  # equal views: image-shaped
    batcher, imsz, _ = tr.gather_training_rays_lazy(types.SimpleNamespace(), {"irregular_shape": False}, torch.stack([imgs[0], imgs[2]]), cfg,
                                                    [0, 1], cfg_train, poses[[0, 2]], HW[[0, 2]], np.stack([Ks[0], Ks[0]]), {}, device="cpu")
    assert batcher.image_shape == (2, 6, 9) and imsz == [1, 1]


class _HalfPlane:
    """a stand-in for the model's filter: the rays whose direction's x component is above the view's mean survive (view 1: none)"""
    def __init__(self, drop_view_origin):
        self.drop = drop_view_origin

    def hit_coarse_geo(self, rays_o, rays_d, **kw):
        assert kw == {"near": 0.2}
        if torch.equal(rays_o[0, 0], self.drop):
            return torch.zeros(rays_o.shape[:-1], dtype=torch.bool)
        return rays_d[..., 0] > rays_d[..., 0].mean()


def test_restrict_keeps_the_rows_of_the_mask_cache_sampler():
    from unboundednerfpytorch_amd import train_rays as tr
    from unboundednerfpytorch_amd.dvgo_render import get_training_rays_in_maskcache_sampling
    imgs, poses, HW, Ks = scene()
    flags = dict(ndc=False, inverse_y=False, flip_x=False, flip_y=False)
    model = _HalfPlane(poses[1, :3, 3].clone())
    want = get_training_rays_in_maskcache_sampling(imgs, poses, [tuple(int(x) for x in hw) for hw in HW], Ks, model=model,
                                                   render_kwargs={"near": 0.2}, **flags)
    b = tr.RayBatcher.from_views(imgs, poses, HW, Ks, with_index=False, **flags)
    imsz = b.restrict(model, {"near": 0.2})
    assert imsz == [int(x) for x in want[4]] and imsz[1] == 0 and 0 < sum(imsz) < b.total and len(b) == sum(imsz)
    got = b.batch(torch.arange(len(b)))
    for a, w in zip(got[:4], want[:4]):
        assert torch.equal(a, w)
    sel = torch.tensor([len(b) - 1, 0, 0, 3])
    assert torch.equal(b.batch(sel)[1], want[1][sel])


def test_uint8_store_takes_exact_multiples_of_one_255th_only():
    from unboundednerfpytorch_amd import train_rays as tr
    _, poses, HW, Ks = scene()
    rs = np.random.RandomState(7)
    raw = [rs.randint(0, 256, (int(h), int(w), 3)).astype(np.uint8) for h, w in HW]
    raw[0].reshape(-1)[:] = np.arange(162)            # every level at least once: 162 values in view 0, the rest in view 2
    raw[2].reshape(-1)[:94] = np.arange(162, 256)
    as_float = [torch.from_numpy((u / 255.).astype(np.float32)) for u in raw]           # the loaders' conversion
    every = torch.arange(sum(u.shape[0] * u.shape[1] for u in raw))
    want = tr.RayBatcher.from_views(as_float, poses.clone(), HW, Ks, with_index=True, **FLAGS).batch(every)
    for images in (as_float, [torch.from_numpy(u) for u in raw]):
        b = tr.RayBatcher.from_views(images, poses.clone(), HW, Ks, with_index=True, store="uint8", **FLAGS)
        assert b.images.dtype == torch.uint8 and b.resident_bytes() == len(every) * 3 + 96 * 3 + 8 * 4
        for a, w in zip(b.batch(every), want):
            assert torch.equal(a, w)
    bad = [x.clone() for x in as_float]
    bad[1][2, 3, 1] = 0.5
    with pytest.raises(ValueError):
        tr.RayBatcher.from_views(bad, poses.clone(), HW, Ks, with_index=True, store="uint8", **FLAGS)
