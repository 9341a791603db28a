"""Ray-batch side of the training loop (run_train.py:129-147,203-247).

The reference prepares ALL training rays once -- `FourierGridModel.gather_training_rays`
(FourierGrid_model.py:298-333) -> `FourierGrid_get_training_rays` (:264-296) / `dvgo.get_training_rays_flatten`
(dvgo.py:594-616) / `dvgo.get_training_rays` (:562-590) / `dvgo.get_training_rays_in_maskcache_sampling` (:619-657) -- and
draws N_rand of them per iteration with `batch_indices_generator` (dvgo.py:660-668) or `torch.randint`
(run_train.py:203-236), copying the batch to the GPU when `load2gpu_on_the_fly` (run_train.py:238-245).

Same functions, same return tuples and the same random streams here (numpy permutation for the sampler, torch.randint for
the 'random' mode), with the rays produced by the one-kernel `fourier_render.get_rays_of_a_view` when the poses live on the
GPU.  On an MI355X the natural set-up is `load2gpu_on_the_fly = False`: 250 full-HD views are 500 M rays x 48 B = 25 GB of
the 288 GB, so the ray table stays resident and a batch is four device-side row gathers -- no per-iteration H2D copy.
NDC (forward-facing) ray tables -- cfg.data.ndc, the DirectMPIGO path (mpi_model.py) -- come from the functions of their own,
`get_training_rays_ndc` / `get_training_rays_flatten_ndc`; the four functions above refuse ndc=True.

Also the two ray-preparation utilities the models and DirectVoxGORenderer share, `voxel_count_views` and `hit_coarse_geo`: on the
package's own ops and float32 device rays each is a kernel of its own per image (ugrid_count_views_accumulate / _commit,
ugrid_hit_coarse_geo: no materialised samples, no autograd, no host read); FUSED_SETUP = False, an injected back-end or CPU
tensors take the composed paths."""
import numpy as np
import torch

from .fourier_render import get_rays_of_a_view

FOURIERGRID_DATASETS = ("waymo", "mega", "nerfpp")      # FourierGrid_model.py:307
FUSED_SETUP = True      # voxel_count_views / hit_coarse_geo on their fused kernels where they apply (False: the composed paths, the A/B)


_NDC = object()


def _rays(H, W, K, c2w, ndc, inverse_y, flip_x, flip_y, device):
    if ndc is _NDC:                  # (only the NDC functions below pass it; a caller's ndc=True is refused)
        ndc = True
    elif ndc:
        raise NotImplementedError("NDC ray tables are built by get_training_rays_ndc / get_training_rays_flatten_ndc "
                                  "(the DirectMPIGO path, mpi_model.py)")
    c2w = torch.as_tensor(c2w, dtype=torch.float32)
    if device.type == "cuda":
        c2w = c2w.to(device)         # device-resident pose: ONE kernel per view (ugrid_rays_of_a_view / _ndc)
    o, d, v = get_rays_of_a_view(int(H), int(W), K, c2w, inverse_y=inverse_y, flip_x=flip_x, flip_y=flip_y, ndc=bool(ndc))
    return o.to(device), d.to(device), v.to(device)


@torch.no_grad()
def get_training_rays(rgb_tr, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y):
    """dvgo.get_training_rays (dvgo.py:562-590): equal-sized views, rays kept as [N,H,W,3]."""
    assert len(np.unique(np.asarray(HW), axis=0)) == 1
    assert len(np.unique(np.asarray(Ks).reshape(len(Ks), -1), axis=0)) == 1
    assert len(rgb_tr) == len(train_poses) and len(rgb_tr) == len(Ks) and len(rgb_tr) == len(HW)
    H, W = (int(x) for x in HW[0])
    K = Ks[0]
    dev = rgb_tr.device
    rays_o_tr = torch.zeros([len(rgb_tr), H, W, 3], device=dev)
    rays_d_tr, viewdirs_tr = torch.zeros_like(rays_o_tr), torch.zeros_like(rays_o_tr)
    for i, c2w in enumerate(train_poses):
        o, d, v = _rays(H, W, K, c2w, ndc, inverse_y, flip_x, flip_y, dev)
        rays_o_tr[i].copy_(o)
        rays_d_tr[i].copy_(d)
        viewdirs_tr[i].copy_(v)
    return rgb_tr, rays_o_tr, rays_d_tr, viewdirs_tr, [1] * len(rgb_tr)


def _flatten(rgb_tr_ori, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y, with_index):
    assert len(rgb_tr_ori) == len(train_poses) and len(rgb_tr_ori) == len(Ks) and len(rgb_tr_ori) == len(HW)
    dev = rgb_tr_ori[0].device
    total = sum(im.shape[0] * im.shape[1] for im in rgb_tr_ori)
    rgb_tr = torch.zeros([total, 3], device=dev)
    rays_o_tr, rays_d_tr, viewdirs_tr = torch.zeros_like(rgb_tr), torch.zeros_like(rgb_tr), torch.zeros_like(rgb_tr)
    indexs_tr = torch.zeros_like(rgb_tr) if with_index else None       # image index, float [N,3] like the reference
    imsz, top = [], 0
    for cur, (c2w, img, (H, W), K) in enumerate(zip(train_poses, rgb_tr_ori, HW, Ks)):
        H, W = int(H), int(W)
        assert tuple(img.shape[:2]) == (H, W)
        o, d, v = _rays(H, W, K, c2w, ndc, inverse_y, flip_x, flip_y, dev)
        n = H * W
        rgb_tr[top:top + n].copy_(img.flatten(0, 1))
        rays_o_tr[top:top + n].copy_(o.flatten(0, 1))
        rays_d_tr[top:top + n].copy_(d.flatten(0, 1))
        viewdirs_tr[top:top + n].copy_(v.flatten(0, 1))
        if with_index:
            indexs_tr[top:top + n] = float(cur)
        imsz.append(n)
        top += n
    assert top == total
    return rgb_tr, rays_o_tr, rays_d_tr, viewdirs_tr, indexs_tr, imsz


@torch.no_grad()
def get_training_rays_flatten(rgb_tr_ori, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y):
    """dvgo.get_training_rays_flatten (dvgo.py:594-616): views of any size, all pixels, flattened to [N,3]."""
    rgb, o, d, v, _, imsz = _flatten(rgb_tr_ori, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y, False)
    return rgb, o, d, v, imsz


@torch.no_grad()
def get_training_rays_ndc(rgb_tr, train_poses, HW, Ks, inverse_y, flip_x, flip_y):
    """dvgo.get_training_rays(ndc=True) (dvgo.py:562-590): rays_o / rays_d in the forward-facing NDC space (ndc_rays with near = 1),
    viewdirs the world directions -- the ray table of DirectMPIGO's 'random' sampler (configs/llff)."""
    return get_training_rays(rgb_tr, train_poses, HW, Ks, _NDC, inverse_y, flip_x, flip_y)


@torch.no_grad()
def get_training_rays_flatten_ndc(rgb_tr_ori, train_poses, HW, Ks, inverse_y, flip_x, flip_y):
    """dvgo.get_training_rays_flatten(ndc=True) (dvgo.py:594-616)"""
    rgb, o, d, v, _, imsz = _flatten(rgb_tr_ori, train_poses, HW, Ks, _NDC, inverse_y, flip_x, flip_y, False)
    return rgb, o, d, v, imsz


@torch.no_grad()
def FourierGrid_get_training_rays(rgb_tr_ori, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y, pos_emb=None):
    """FourierGridModel.FourierGrid_get_training_rays (FourierGrid_model.py:264-296): the flattened rays plus the image
    index of every ray; pos_emb (the model's optional pose refinement) is added to the camera centres IN PLACE, as the
    reference does."""
    if pos_emb is not None:
        train_poses[:, :3, 3] = train_poses[:, :3, 3] + pos_emb
    return _flatten(rgb_tr_ori, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y, True)


def batch_indices_generator(N, BS):
    """dvgo.batch_indices_generator (dvgo.py:660-668): epochs of a numpy permutation cut into BS-sized index batches; an
    incomplete tail is dropped and a new permutation drawn.  Same numpy random stream as the reference."""
    idx, top = torch.LongTensor(np.random.permutation(N)), 0
    while True:
        if top + BS > N:
            idx, top = torch.LongTensor(np.random.permutation(N)), 0
        yield idx[top:top + BS]
        top += BS


def _get(cfg, name, default=None):
    return cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)


def gather_training_rays(model, data_dict, images, cfg, i_train, cfg_train, poses, HW, Ks, render_kwargs, device=None):
    """FourierGridModel.gather_training_rays (FourierGrid_model.py:298-333).  cfg / cfg.data / cfg_train: attribute objects
    or dicts.  Returns (rgb_tr, rays_o_tr, rays_d_tr, viewdirs_tr, indexs_train, imsz, batch_index_sampler)."""
    data = _get(cfg, 'data')
    if device is None:
        device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    store = torch.device('cpu') if _get(data, 'load2gpu_on_the_fly', False) else torch.device(device)
    if _get(data_dict, 'irregular_shape'):
        rgb_tr_ori = [images[i].to(store) for i in i_train]
    else:
        rgb_tr_ori = images[i_train].to(store)
    kw = dict(train_poses=poses[i_train], HW=HW[i_train], Ks=Ks[i_train], ndc=_get(data, 'ndc', False),
              inverse_y=_get(data, 'inverse_y', False), flip_x=_get(data, 'flip_x', False), flip_y=_get(data, 'flip_y', False))
    indexs_train = None
    sampler = _get(cfg_train, 'ray_sampler')
    if _get(data, 'dataset_type') in FOURIERGRID_DATASETS or _get(cfg, 'model') == 'FourierGrid':
        rgb_tr, rays_o_tr, rays_d_tr, viewdirs_tr, indexs_train, imsz = FourierGrid_get_training_rays(
            rgb_tr_ori=rgb_tr_ori, pos_emb=getattr(model, 'pos_emb', None), **kw)
    elif sampler == 'in_maskcache':
        from .dvgo_render import get_training_rays_in_maskcache_sampling
        rgb_tr, rays_o_tr, rays_d_tr, viewdirs_tr, imsz = get_training_rays_in_maskcache_sampling(
            rgb_tr_ori=rgb_tr_ori, model=model, render_kwargs=render_kwargs, **kw)
    elif sampler == 'flatten':
        rgb_tr, rays_o_tr, rays_d_tr, viewdirs_tr, imsz = get_training_rays_flatten(rgb_tr_ori=rgb_tr_ori, **kw)
    else:
        rgb_tr, rays_o_tr, rays_d_tr, viewdirs_tr, imsz = get_training_rays(rgb_tr=rgb_tr_ori, **kw)
    index_generator = batch_indices_generator(len(rgb_tr), _get(cfg_train, 'N_rand'))
    return rgb_tr, rays_o_tr, rays_d_tr, viewdirs_tr, indexs_train, imsz, (lambda: next(index_generator))


def sample_batch(cfg_train, rgb_tr, rays_o_tr, rays_d_tr, viewdirs_tr, indexs_tr, batch_index_sampler, device=None,
                 load2gpu_on_the_fly=False):
    """One iteration's ray batch (run_train.py:203-245): returns (target, rays_o, rays_d, viewdirs, indexs).
    'flatten' / 'in_maskcache': rows chosen by batch_index_sampler(); 'random': torch.randint over the leading dims of
    the (image-shaped or flattened) ray table, on its device -- the same draws in the same order as the reference.
    With load2gpu_on_the_fly the five tensors are copied to `device`; with a resident table (the MI355X set-up) the index
    tensor goes to the table's device and the batch is four row gathers there."""
    sampler = _get(cfg_train, 'ray_sampler')
    n_rand = _get(cfg_train, 'N_rand')
    if sampler in ('flatten', 'in_maskcache'):
        sel = batch_index_sampler()
        if sel.device != rgb_tr.device:
            sel = sel.to(rgb_tr.device, non_blocking=True)
        sel = (sel,)
    elif sampler == 'random':
        if rgb_tr.dim() != 2:
            sel = tuple(torch.randint(rgb_tr.shape[k], [n_rand], device=rgb_tr.device) for k in range(3))
        else:
            sel_b = torch.randint(rgb_tr.shape[0], [n_rand], device=rgb_tr.device)
            torch.randint(rgb_tr.shape[1], [n_rand], device=rgb_tr.device)       # the reference draws (and ignores) sel_r
            sel = (sel_b,)
    else:
        raise NotImplementedError(sampler)
    out = [t[sel] if t is not None else None for t in (rgb_tr, rays_o_tr, rays_d_tr, viewdirs_tr, indexs_tr)]
    if load2gpu_on_the_fly:
        out = [t.to(device) if t is not None else None for t in out]
    return tuple(out)


def _fused_rays(*rays):
    """the fused set-up kernels take float32 rays that live on the GPU"""
    return FUSED_SETUP and all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 for x in rays)


def _count_n_samples(world_size, stepsize):
    return int(np.linalg.norm(world_size.cpu().numpy().astype(np.float64) + 1) / stepsize) + 1


@torch.no_grad()
def voxel_count_views_fused(xyz_min, xyz_max, voxel_size, world_size, count_shape, rays_o_tr, rays_d_tr, imsz, near, stepsize,
                            downrate=1, irregular_shape=False):
    """voxel_count_views on two kernels per image (ugrid_count_views_accumulate: one lane per ray adds the trilinear footprint of its
    samples into a scratch grid; ugrid_count_views_commit: count += scratch > 1, scratch = 0): the whole image at once, no points
    materialised, no autograd, no host read.  Same images ([::downrate, ::downrate] / the imsz split), same n_samples, and
    stepdist = stepsize * voxel_size formed in float32 like the composed path's; the same sums in another order."""
    from . import _lib
    L = _lib.load()
    dev = xyz_min.device
    far = 1e9
    n_samples = _count_n_samples(world_size, stepsize)
    stepdist = float(stepsize * voxel_size)                  # (the float32 product of the composed path, read back once)
    X, Y, Z = (int(x) for x in world_size.tolist())
    lo, hi = xyz_min.contiguous(), xyz_max.contiguous()
    _lib.require_cuda(("xyz_min", lo), ("xyz_max", hi))
    _lib.require_f32(("xyz_min", lo), ("xyz_max", hi))
    count = torch.zeros(count_shape, device=dev)
    if count.numel() != X * Y * Z:
        raise RuntimeError("voxel_count_views: count_shape %s does not hold world_size %s" % (tuple(count_shape), (X, Y, Z)))
    acc = torch.zeros(X * Y * Z, device=dev)
    with _lib.guard(dev):
        st = _lib.stream_of(count)
        for o_img, d_img in zip(rays_o_tr.split(imsz), rays_d_tr.split(imsz)):
            if not irregular_shape:
                o_img, d_img = o_img[::downrate, ::downrate], d_img[::downrate, ::downrate]
            o, d = o_img.to(dev).reshape(-1, 3).contiguous(), d_img.to(dev).reshape(-1, 3).contiguous()
            _lib.check(L.ugrid_count_views_accumulate(o.data_ptr(), d.data_ptr(), o.shape[0], lo.data_ptr(), hi.data_ptr(), float(near), far,
                                                      stepdist, n_samples, X, Y, Z, acc.data_ptr(), st), "count_views_accumulate")
            _lib.check(L.ugrid_count_views_commit(acc.data_ptr(), count.data_ptr(), X * Y * Z, st), "count_views_commit")
    return count


def voxel_count_views(query, xyz_min, xyz_max, voxel_size, world_size, count_shape, rays_o_tr, rays_d_tr, imsz, near, stepsize,
                      downrate=1, irregular_shape=False):
    """How many training views see each voxel of a plain grid of `world_size` over the box (dvgo.py:247-277,
    FourierGrid_model.py:392-418): per image the trilinear footprint of its rays' samples is scattered into a zero grid -- by
    the backward of `query`, a differentiable lookup (grid.GridQuery.apply or an injected one) -- and a voxel counts as seen
    when it gathered more than 1.  Returns the counts as a float grid of `count_shape` (the model's density grid's).
    With the package's own lookup and float32 rays on the GPU: voxel_count_views_fused."""
    from . import grid as _grid
    # (`==`: every access of a Function's `apply` makes a new bound method; equal ones are the same op)
    if query == _grid.GridQuery.apply and _fused_rays(rays_o_tr, rays_d_tr) and xyz_min.is_cuda:
        return voxel_count_views_fused(xyz_min, xyz_max, voxel_size, world_size, count_shape, rays_o_tr, rays_d_tr, imsz, near, stepsize,
                                       downrate, irregular_shape)
    far = 1e9
    dev = xyz_min.device
    n_samples = _count_n_samples(world_size, stepsize)
    rng = torch.arange(n_samples, device=dev)[None].float()
    count = torch.zeros(count_shape, device=dev)
    for o_img, d_img in zip(rays_o_tr.split(imsz), rays_d_tr.split(imsz)):
        ones = torch.zeros([1, 1] + world_size.tolist(), device=dev).requires_grad_(True)
        if irregular_shape:
            o_chunks, d_chunks = o_img.split(10000), d_img.split(10000)
        else:
            o_chunks = o_img[::downrate, ::downrate].to(dev).flatten(0, -2).split(10000)
            d_chunks = d_img[::downrate, ::downrate].to(dev).flatten(0, -2).split(10000)
        for o, d in zip(o_chunks, d_chunks):
            o, d = o.to(dev), d.to(dev)
            vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
            t_min = torch.minimum((xyz_max - o) / vec, (xyz_min - o) / vec).amax(-1).clamp(min=near, max=far)
            step = stepsize * voxel_size * rng
            pts = o[..., None, :] + d[..., None, :] * (t_min[..., None] + step / d.norm(dim=-1, keepdim=True))[..., None]
            query(ones, pts, xyz_min, xyz_max, 0).sum().backward()
        with torch.no_grad():
            count += (ones.grad > 1)
    return count


@torch.no_grad()
def hit_coarse_geo(ru, rays_o, rays_d, xyz_min, xyz_max, near, stepdist, mask, xyz2ijk_scale, xyz2ijk_shift):
    """bool [...]: does the ray pass through a cell the mask cache marks as possibly occupied? (dvgo.py:291-304)
    ru: the render_utils_cuda module (sample_pts_on_rays, maskcache_lookup) or another implementation of it.
    The package's own module on float32 device rays: ONE kernel, a lane per ray (ugrid_hit_coarse_geo) -- the same bits."""
    far = 1e9
    shape = rays_o.shape[:-1]
    o, d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
    from . import render_utils_cuda as _own
    if ru is _own and _fused_rays(o, d):
        from . import _lib
        small = [xyz_min.contiguous(), xyz_max.contiguous(), xyz2ijk_scale.contiguous(), xyz2ijk_shift.contiguous()]
        named = list(zip(("xyz_min", "xyz_max", "xyz2ijk_scale", "xyz2ijk_shift"), small))
        _lib.require_cuda(*named, ("mask", mask))
        _lib.require_f32(*named)
        if mask.dtype != torch.bool or mask.dim() != 3 or any(x.device != o.device for x in small + [mask]):
            raise RuntimeError("hit_coarse_geo: mask must be a bool tensor [mi,mj,mk] on the rays' device, like the box and the scale / shift")
        mask = mask.contiguous()
        hit = torch.empty(o.shape[0], dtype=torch.bool, device=o.device)
        with _lib.guard(o.device):
            _lib.check(_lib.load().ugrid_hit_coarse_geo(o.data_ptr(), d.data_ptr(), o.shape[0], small[0].data_ptr(), small[1].data_ptr(),
                                                        float(near), far, float(stepdist), mask.data_ptr(), *mask.shape,
                                                        small[2].data_ptr(), small[3].data_ptr(), hit.data_ptr(), _lib.stream_of(o)),
                       "hit_coarse_geo")
        return hit.reshape(shape)
    pts, outbbox, ray_id = ru.sample_pts_on_rays(o, d, xyz_min, xyz_max, near, far, stepdist)[:3]
    inb = ~outbbox
    occ = ru.maskcache_lookup(mask, pts[inb].contiguous(), xyz2ijk_scale, xyz2ijk_shift)
    hit = torch.zeros(o.shape[0], dtype=torch.bool, device=o.device)
    hit[ray_id[inb][occ]] = True
    return hit.reshape(shape)
