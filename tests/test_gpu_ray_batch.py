"""ugrid_ray_batch (train_rays.RayBatcher.batch on the GPU) against the ray tables it replaces, built on the same device by the
per-view kernel: every output bit for bit (torch.equal) -- the batch kernel calls the per-ray leaves of k_rays_of_a_view /
k_rays_of_a_view_ndc --, the samplers' random streams, the mask-cache sampler, guarded output buffers and the memory condition
that is the point of the feature."""
import itertools

import numpy as np
import pytest
import torch

import synth
from test_gpu_voxgo_train import build, DVGO_CASES

pytestmark = pytest.mark.gpu
SIZES = [(5, 7), (4, 9), (6, 6)]
ALL_FLAGS = [dict(inverse_y=a, flip_x=b, flip_y=c) for a, b, c in itertools.product((False, True), repeat=3)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def views(dev):
    """three views of unequal size with intrinsics of their own; near-identity poses (so that the NDC rays are finite too)"""
    g = torch.Generator().manual_seed(21)
    imgs = [torch.rand(h, w, 3, generator=g).to(dev) for h, w in SIZES]
    poses = torch.eye(4)[:3].repeat(3, 1, 1) + 0.1 * torch.randn(3, 3, 4, generator=g)
    Ks = np.array([[[31.0 + 4 * i, 0, w / 2.0 + 0.25 * i], [0, 33.5 - 3 * i, h / 2.0 - 0.5 * i], [0, 0, 1]] for i, (h, w) in enumerate(SIZES)],
                  dtype=np.float32)
    return imgs, poses, np.array(SIZES), Ks


@pytest.fixture(scope="module")
def index_lists(dev):
    """every pixel once in a permuted order, 40 duplicates, the first and last pixel of every view (the search's boundaries); and
    lists of 1, 257 (more than one block, with repeats) and 0 rows"""
    rs = np.random.RandomState(8)
    counts = [h * w for h, w in SIZES]
    total = sum(counts)
    start = np.concatenate([[0], np.cumsum(counts)])
    edges = np.stack([start[:-1], start[1:] - 1], 1).reshape(-1)
    full = np.concatenate([rs.permutation(total), rs.randint(0, total, 40), edges])
    lists = [full, np.array([total - 1]), rs.randint(0, total, 257), np.zeros(0, dtype=np.int64)]
    return [torch.from_numpy(x.astype(np.int64)).to(dev) for x in lists]


@pytest.mark.parametrize("with_index", [False, True])
def test_batch_rows_equal_the_table_rows_bit_for_bit(views, index_lists, with_index):
    from unboundednerfpytorch_amd import train_rays as tr
    imgs, poses, HW, Ks = views
    for flags in ALL_FLAGS:
        table = tr._flatten(imgs, poses, HW, Ks, False, with_index=with_index, **flags)
        b = tr.RayBatcher.from_views(imgs, poses, HW, Ks, ndc=False, with_index=with_index, **flags)
        assert b.images.is_cuda and len(b) == table[0].shape[0] == 107 and b.imsz == table[5]
        for sel in index_lists:
            out = b.batch(sel)
            assert len(out) == 5 and (out[4] is not None) == with_index
            for got, want in zip(out, table[:5]):
                if want is None:
                    assert got is None
                    continue
                assert got.shape == (sel.numel(), 3) and got.dtype == torch.float32 and got.is_contiguous()
                assert torch.equal(got, want[sel]), (flags, sel.numel())
    if with_index:      # the first and last pixel of every view find their own view
        assert b.batch(index_lists[0])[4][-6:].cpu().tolist() == [[float(i)] * 3 for i in (0, 0, 1, 1, 2, 2)]


def test_ndc_batch_rows_equal_the_ndc_table_rows_bit_for_bit(views, index_lists):
    from unboundednerfpytorch_amd import train_rays as tr
    imgs, poses, HW, Ks = views
    for flags in ALL_FLAGS:
        table = tr.get_training_rays_flatten_ndc(imgs, poses, HW, Ks, **flags)
        assert all(bool(torch.isfinite(t).all()) for t in table[:4])
        b = tr.RayBatcher.from_views(imgs, poses, HW, Ks, ndc=True, with_index=False, **flags)
        for sel in index_lists:
            out = b.batch(sel)
            assert out[4] is None
            for got, want in zip(out[:4], table[:4]):
                assert got.shape == (sel.numel(), 3) and torch.equal(got, want[sel]), (flags, sel.numel())
    # the NDC origins differ from the world ones: the other leaf really ran
    world = tr.RayBatcher.from_views(imgs, poses, HW, Ks, ndc=False, with_index=False, **ALL_FLAGS[-1]).batch(index_lists[0])
    assert not torch.equal(world[1], out[1]) and torch.equal(world[3], b.batch(index_lists[0])[3])


def test_uint8_store_gives_the_rows_of_the_float_store(views, index_lists, dev):
    from unboundednerfpytorch_amd import train_rays as tr
    _, poses, HW, Ks = views
    rs = np.random.RandomState(3)
    raw = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]
    raw[0].reshape(-1)[:] = np.arange(105)            # every level at least once
    raw[1].reshape(-1)[:] = np.arange(105, 213)
    raw[2].reshape(-1)[:43] = np.arange(213, 256)
    as_float = [torch.from_numpy((u / 255.).astype(np.float32)).to(dev) for u in raw]         # the loaders' conversion
    kw = dict(ndc=False, inverse_y=True, flip_x=False, flip_y=True, with_index=True)
    f = tr.RayBatcher.from_views(as_float, poses, HW, Ks, **kw)
    for images in ([torch.from_numpy(u).to(dev) for u in raw], as_float, [torch.from_numpy(u) for u in raw]):
        u = tr.RayBatcher.from_views(images, poses, HW, Ks, store="uint8", device=dev, **kw)
        assert u.images.dtype == torch.uint8 and u.images.is_cuda and u.resident_bytes() == 107 * 3 + 3 * 96 + 4 * 8
        for sel in index_lists:
            for a, b in zip(u.batch(sel), f.batch(sel)):
                assert torch.equal(a, b)
    assert torch.equal(f.batch(torch.arange(107, device=dev))[0], torch.cat([x.reshape(-1, 3) for x in as_float]))
    with pytest.raises(ValueError):
        f.batch(torch.arange(4))                      # a host index for a device batcher


def test_random_sampler_makes_the_draws_of_sample_batch(dev):
    from unboundednerfpytorch_amd import train_rays as tr
    g = torch.Generator().manual_seed(22)
    rgb = torch.rand(2, 6, 9, 3, generator=g).to(dev)
    poses = torch.eye(4)[:3].repeat(2, 1, 1) + 0.1 * torch.randn(2, 3, 4, generator=g)
    HW = np.array([(6, 9), (6, 9)])
    K = np.array([[40.0, 0, 4.5], [0, 41.0, 3.0], [0, 0, 1]], dtype=np.float32)
    Ks = np.stack([K, K])
    flags = dict(inverse_y=False, flip_x=True, flip_y=False)
    cfg = {"ray_sampler": "random", "N_rand": 64}
    shaped_table = tr.get_training_rays(rgb, poses, HW, Ks, False, **flags)
    flat_table = tr.get_training_rays_flatten(rgb, poses, HW, Ks, False, **flags)
    shaped = tr.RayBatcher.from_views(rgb, poses, HW, Ks, ndc=False, with_index=False, image_shaped=True, **flags)
    flat = tr.RayBatcher.from_views(rgb, poses, HW, Ks, ndc=False, with_index=False, **flags)
    assert shaped.images.data_ptr() == rgb.data_ptr()            # a resident image tensor is kept, not copied
    for table, batcher in ((shaped_table, shaped), (flat_table, flat)):
        torch.manual_seed(9)
        want = [tr.sample_batch(cfg, *table[:4], None, None) for _ in range(2)]
        state = torch.cuda.get_rng_state(dev)
        torch.manual_seed(9)
        got = [tr.sample_batch_lazy(cfg, batcher, None) for _ in range(2)]
        assert torch.equal(torch.cuda.get_rng_state(dev), state)
        for w, g_ in zip(want, got):
            assert g_[4] is None and all(a.shape == (64, 3) and torch.equal(a, b) for a, b in zip(g_[:4], w[:4]))
        assert not torch.equal(got[0][0], got[1][0])


def test_flatten_sampler_gives_the_batches_of_the_table_path(views, dev):
    from unboundednerfpytorch_amd import train_rays as tr
    imgs, poses, HW, Ks = views
    kw = dict(inverse_y=True, flip_x=False, flip_y=True)
    cfg = {"ray_sampler": "flatten", "N_rand": 32}     # 107 rows: three batches an epoch, the tail of 11 dropped
    table = tr.FourierGrid_get_training_rays(imgs, poses.clone(), HW, Ks, False, **kw)
    b = tr.RayBatcher.from_views(imgs, poses.clone(), HW, Ks, ndc=False, with_index=True, **kw)
    np.random.seed(13)
    host = tr.batch_indices_generator(107, 32)
    want = [tr.sample_batch(cfg, *table[:5], lambda: next(host)) for _ in range(7)]
    np.random.seed(13)
    device = tr.device_batch_indices_generator(len(b), 32, dev)
    seen = []

    def sampler():
        seen.append(next(device))
        return seen[-1]
    got = [tr.sample_batch_lazy(cfg, b, sampler) for _ in range(7)]
    assert all(s.is_cuda and s.dtype == torch.int64 for s in seen)
    assert len(set(torch.cat(seen[:3]).tolist())) == 96 and len(set(torch.cat(seen[3:6]).tolist())) == 96
    for w, g_ in zip(want, got):
        assert all(torch.equal(a, b_) for a, b_ in zip(g_, w))


def _look(eye, fwd):
    fwd = np.asarray(fwd, dtype=np.float64) / np.linalg.norm(fwd)
    right = np.cross(fwd, [0.0, 0.0, 1.0]); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    return np.stack([right, up, -fwd, np.asarray(eye, dtype=np.float64)], axis=1).astype(np.float32)


def test_restrict_keeps_the_rows_of_the_mask_cache_sampler(dev):
    """a DirectVoxGO model with a full mask cache: a view from the middle of the box keeps every ray, a view that looks away from
    the box keeps none, the views of synth.dvgo_views keep the rays that meet the box"""
    from unboundednerfpytorch_amd import train_rays as tr
    from unboundednerfpytorch_amd.dvgo_render import get_training_rays_in_maskcache_sampling
    m = build("dvgo", DVGO_CASES[0], dev)[0]
    with torch.no_grad():
        m.mask_cache.mask.fill_(True)
    H, W, K, poses = synth.dvgo_views()
    poses = [poses[0], _look([2.6, 0.4, 0.2], [1.0, 0.1, 0.0]), _look([0.0, 0.0, 0.0], [0.3, 1.0, 0.1]), poses[2]]
    poses = torch.from_numpy(np.stack(poses))
    n = len(poses)
    Ks = np.stack([K * np.array([[1.0 + 0.1 * i], [1.0], [1.0]], dtype=np.float32) for i in range(n)])      # another focal a view
    imgs = [torch.from_numpy(synth.uniform(700 + i, H * W * 3).reshape(H, W, 3)).to(dev) for i in range(n)]
    rk = dict(near=0.2, far=6.0, stepsize=0.5)
    flags = dict(ndc=False, inverse_y=False, flip_x=False, flip_y=False)
    want = get_training_rays_in_maskcache_sampling(imgs, poses, [(H, W)] * n, Ks, model=m, render_kwargs=rk, **flags)
    b = tr.RayBatcher.from_views(imgs, poses, [(H, W)] * n, Ks, with_index=False, **flags)
    imsz = b.restrict(m, rk)
    assert imsz == [int(x) for x in want[4]], (imsz, want[4])
    assert imsz[1] == 0 and imsz[2] == H * W and 0 < imsz[0] and len(b) == sum(imsz) == want[0].shape[0]
    assert b.rows.dtype == torch.int64 and b.rows.is_cuda
    got = b.batch(torch.arange(len(b), device=dev))
    for a, w in zip(got[:4], want[:4]):
        assert torch.equal(a, w)
    sel = torch.tensor([len(b) - 1, 0, 5, 5], device=dev)
    assert all(torch.equal(a, w[sel]) for a, w in zip(b.batch(sel)[:4], want[:4]))
    # nothing survives: an empty row list, zero counts, empty batches
    with torch.no_grad():
        m.mask_cache.mask.fill_(False)
    assert b.restrict(m, rk) == [0] * n and len(b) == 0 and b.rows.shape == (0,)
    assert [tuple(t.shape) for t in b.batch(torch.zeros(0, dtype=torch.int64, device=dev))[:4]] == [(0, 3)] * 4


def test_the_kernel_writes_inside_its_output_buffers_only(views, index_lists, dev):
    """the C entry point on five [257,3] buffers carved out of canary-filled allocations: the rows are those of batch(), the
    canaries on both sides of every buffer are intact; n = 0 launches nothing"""
    from unboundednerfpytorch_amd import _lib, train_rays as tr
    imgs, poses, HW, Ks = views
    b = tr.RayBatcher.from_views(imgs, poses, HW, Ks, ndc=False, inverse_y=True, flip_x=True, flip_y=False, with_index=True)
    sel = index_lists[2]
    n, pad, canary = 257, 64, -7.25
    big = torch.full((5, pad + 3 * n + pad), canary, device=dev)
    ptrs = [big[i].data_ptr() + 4 * pad for i in range(5)]
    L = _lib.load()

    def call(count):
        return L.ugrid_ray_batch(b.cams.data_ptr(), b.view_start.data_ptr(), b.n_views, sel.data_ptr(), count, b.images.data_ptr(), 0,
                                 1, 1, 0, 1, 0, 1.0, *ptrs, _lib.stream_of(sel))
    assert call(0) == 0
    torch.cuda.synchronize()
    assert bool((big == canary).all())
    assert call(n) == 0
    torch.cuda.synchronize()
    assert bool((big[:, :pad] == canary).all()) and bool((big[:, pad + 3 * n:] == canary).all())
    for i, want in enumerate(b.batch(sel)):
        assert torch.equal(big[i, pad:pad + 3 * n].reshape(n, 3), want)
    assert call(-3) == 0 and L.ugrid_ray_batch(None, None, 0, None, 5, None, 0, 0, 0, 0, 1, 0, 1.0, *ptrs, None) != 0   # refused on the host


@pytest.mark.parametrize("restricted", [False, True])
def test_resident_memory_is_the_images_not_a_ray_table(dev, restricted):
    """Six float views of 96 x 128: the images are 884,736 B, a ray table would add four (five with the index) times that.  The
    rise of the allocator's peak across from_views and three batches of 1024 stays under the image bytes + 1 MB (camera table,
    prefix, batch outputs, the epoch's permutation, allocator rounding); with restrict() one more view's rays (o, d, viewdirs:
    3 x 147,456 B) while the filter runs.  A condition, not a measurement."""
    from unboundednerfpytorch_amd import train_rays as tr
    H, W, n = 96, 128, 6
    image_bytes = n * H * W * 12
    assert image_bytes == 884736
    g = torch.Generator().manual_seed(4)
    imgs = [torch.rand(H, W, 3, generator=g) for _ in range(n)]               # on the host: the resident copy is from_views'
    _, _, K, p3 = synth.dvgo_views()
    poses = torch.from_numpy(np.stack([p3[i % 3] for i in range(n)]))
    Ks = np.stack([K * np.array([[8.0], [8.0], [1.0]], dtype=np.float32)] * n)
    m = build("dvgo", DVGO_CASES[0], dev)[0] if restricted else None
    if restricted:
        with torch.no_grad():
            m.mask_cache.mask.fill_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    b = tr.RayBatcher.from_views(imgs, poses, [(H, W)] * n, Ks, ndc=False, inverse_y=False, flip_x=False, flip_y=False,
                                 with_index=not restricted, device=dev)
    if restricted:
        imsz = b.restrict(m, dict(near=0.2, far=6.0, stepsize=0.5))
        assert 0 < sum(imsz) == len(b) <= n * H * W
    np.random.seed(1)
    sampler = tr.device_batch_indices_generator(len(b), 1024, dev)
    keep = [tr.sample_batch_lazy({"ray_sampler": "flatten", "N_rand": 1024}, b, lambda: next(sampler)) for _ in range(3)]
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - base
    allowed = image_bytes + (1 << 20) + (3 * H * W * 12 if restricted else 0)
    print("peak rise %d B, allowed %d B, images %d B" % (rise, allowed, image_bytes))
    assert keep[2][0].shape == (1024, 3) and image_bytes <= rise < allowed, (rise, allowed)
