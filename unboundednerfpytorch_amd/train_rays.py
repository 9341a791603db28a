"""Ray-batch side of the training loop (run_train.py:129-147,203-247).

The reference prepares ALL training rays once -- `FourierGridModel.gather_training_rays`
(FourierGrid_model.py:298-333) -> `FourierGrid_get_training_rays` (:264-296) / `dvgo.get_training_rays_flatten`
(dvgo.py:594-616) / `dvgo.get_training_rays` (:562-590) / `dvgo.get_training_rays_in_maskcache_sampling` (:619-657) -- and
draws N_rand of them per iteration with `batch_indices_generator` (dvgo.py:660-668) or `torch.randint`
(run_train.py:203-236), copying the batch to the GPU when `load2gpu_on_the_fly` (run_train.py:238-245).

Same functions, same return tuples and the same random streams here (numpy permutation for the sampler, torch.randint for
the 'random' mode), with the rays produced by the one-kernel `fourier_render.get_rays_of_a_view` when the poses live on the
GPU.  Where the table fits an MI355X the set-up is `load2gpu_on_the_fly = False`: 250 full-HD views are 500 M rays x 48 B =
25 GB of the 288 GB (60 B a ray with FourierGrid's index triple: 31 GB), so the ray table stays resident and a batch is four
or five device-side row gathers -- no per-iteration H2D copy.  That is Tanks and Temples.  The table stops fitting long before
the scenes the project is named for: at 60 B a pixel the ~1.9 k views of ~1 M pixels of configs/mega/building are ~115 GB, and
the ~5 k views of quad no longer fit a card at all -- the reference answers with load2gpu_on_the_fly = True, CPU tables and
an H2D copy of five tensors every iteration.  For those there is `RayBatcher` (gather_training_rays_lazy /
sample_batch_lazy): only the images (12 B a pixel, or 3 B as 8-bit) and a 96 B record per view stay resident, and a batch is
ONE kernel (ugrid_ray_batch) that forms each row's ray from its pixel index with the arithmetic of the ray-generation kernel.
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


# ugrid_ray_cam (include/ugrid_hip.h): one 96-byte record per view
RAY_CAM = np.dtype([("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("W", "<i4"), ("H", "<i4"), ("c2w", "<f4", (12,)),
                    ("kx", "<f4"), ("ky", "<f4"), ("reserved", "<f4", (4,))])
assert RAY_CAM.itemsize == 96
_STORES = {"float32": (torch.float32, 0), "uint8": (torch.uint8, 1)}      # store -> (dtype, image_kind of ugrid_ray_batch)


def _as_uint8(img):
    """An image for the 8-bit store: uint8 as it is; a float image only if every value is exactly k/255 in float32, the value of the
    loaders' (img / 255.).astype(np.float32) -- what ugrid_ray_batch gives back."""
    if img.dtype == torch.uint8:
        return img
    if not img.dtype.is_floating_point:
        raise ValueError("store='uint8' takes uint8 images or float images that hold k/255 exactly (got %s)" % img.dtype)
    q = (img.double() * 255.).round().clamp_(0, 255).to(torch.uint8)
    if not torch.equal((q.double() / 255.).to(torch.float32), img.to(torch.float32)):
        raise ValueError("store='uint8': the image holds values that are not k/255 in float32; keep it in the float32 store")
    return q


class RayBatcher:
    """The training views as a pose table: the flattened images (float32 [total,3], or uint8), one ugrid_ray_cam record per view and
    the prefix of the views' pixel counts -- nothing else of size [total,3].  `batch(index)` produces the rows that the tables of
    get_training_rays_flatten / FourierGrid_get_training_rays / get_training_rays(_flatten)_ndc hold at the global pixel indices
    `index` (views in order, pixels in image order): on the GPU ONE kernel, ugrid_ray_batch, bit for bit the rows of a table built
    on that device; on the CPU a torch composition over fourier_render.get_rays_of_pixel_index (host-side utility and tests).
    image_shape = (N, H, W) marks equal-sized views sampled like get_training_rays' image-shaped table ('random' draws three
    indices); after restrict() an index addresses the surviving rows."""

    def __init__(self, images, cams, view_start, poses, HW, Ks, ndc, inverse_y, flip_x, flip_y, with_index, store, image_shape):
        self.images, self.cams, self.view_start = images, cams, view_start
        self.poses, self.HW, self.Ks = poses, HW, Ks
        self.ndc, self.inverse_y, self.flip_x, self.flip_y = bool(ndc), bool(inverse_y), bool(flip_x), bool(flip_y)
        self.with_index, self.store, self.image_shape = bool(with_index), store, image_shape
        self.device = images.device
        self.n_views = len(HW)
        self.view_start_host = view_start.cpu()
        self.total = int(self.view_start_host[-1])
        self.rows = None

    @classmethod
    @torch.no_grad()
    def from_views(cls, rgb_tr_ori, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y, with_index, store="float32", pos_emb=None,
                   device=None, image_shaped=False):
        """rgb_tr_ori: [N,H,W,3] or a list of [H,W,3] images; train_poses [N,3|4,4]; pos_emb (the model's pose refinement) is added
        to the camera centres IN PLACE before the table is built, as FourierGrid_get_training_rays does.  ndc=True: the NDC rays
        of get_training_rays_flatten_ndc (near = 1).  image_shaped: equal views and intrinsics, as get_training_rays demands."""
        n_views = len(rgb_tr_ori)
        if not (n_views == len(train_poses) == len(Ks) == len(HW)) or n_views == 0:
            raise ValueError("RayBatcher: %d images, %d poses, %d Ks, %d HW" % (n_views, len(train_poses), len(Ks), len(HW)))
        if store not in _STORES:
            raise ValueError("store must be 'float32' or 'uint8' (got %r)" % (store,))
        dtype = _STORES[store][0]
        device = torch.device(rgb_tr_ori[0].device if device is None else device)
        if pos_emb is not None:
            train_poses[:, :3, 3] = train_poses[:, :3, 3] + pos_emb
        HW = [(int(h), int(w)) for h, w in HW]
        if image_shaped:
            assert len(set(HW)) == 1
            assert len(np.unique(np.stack([np.asarray(torch.as_tensor(K).cpu()) for K in Ks]).reshape(n_views, -1), axis=0)) == 1
        for img, (H, W) in zip(rgb_tr_ori, HW):
            if tuple(img.shape) != (H, W, 3):
                raise ValueError("RayBatcher: an image of shape %s for a %d x %d view" % (tuple(img.shape), H, W))
        start = np.zeros(n_views + 1, dtype=np.int64)
        start[1:] = np.cumsum([h * w for h, w in HW])
        total = int(start[-1])
        whole = torch.is_tensor(rgb_tr_ori) and rgb_tr_ori.device == device and rgb_tr_ori.is_contiguous()
        if whole and rgb_tr_ori.dtype == dtype:      # already resident in the store's type: keep it, flattened
            images = rgb_tr_ori.reshape(total, 3)
        else:
            images = torch.empty([total, 3], dtype=dtype, device=device)
            for img, a, b in zip(rgb_tr_ori, start[:-1], start[1:]):
                images[int(a):int(b)].copy_((_as_uint8(img) if store == "uint8" else img).reshape(-1, 3))
        poses = torch.stack([torch.as_tensor(p, dtype=torch.float32)[:3, :4].cpu() for p in train_poses])
        cams = np.zeros(n_views, dtype=RAY_CAM)
        for i, ((H, W), K) in enumerate(zip(HW, Ks)):
            fx = np.float32(float(K[0][0]))
            cams[i] = (fx, float(K[1][1]), float(K[0][2]), float(K[1][2]), W, H, poses[i].reshape(-1).numpy(),
                       -1. / (W / (2. * float(fx))), -1. / (H / (2. * float(fx))), np.zeros(4))
        cams = torch.from_numpy(cams.view(np.uint8).reshape(n_views, RAY_CAM.itemsize)).to(device)
        shape = (n_views,) + HW[0] if image_shaped else None
        return cls(images, cams, torch.from_numpy(start).to(device), poses, HW, list(Ks), ndc, inverse_y, flip_x, flip_y, with_index,
                   store, shape)

    def __len__(self):
        return self.total if self.rows is None else int(self.rows.numel())

    @property
    def imsz(self):
        """the per-view pixel counts ([1] * N for image-shaped views, like get_training_rays)"""
        if self.image_shape is not None:
            return [1] * self.n_views
        return [h * w for h, w in self.HW]

    def resident_bytes(self):
        return sum(t.numel() * t.element_size() for t in (self.images, self.cams, self.view_start, self.rows) if t is not None)

    @torch.no_grad()
    def batch(self, index):
        """(target, rays_o, rays_d, viewdirs, indexs or None), [n,3] each, for the int64 indices `index` [n] on the batcher's device"""
        if not torch.is_tensor(index) or index.dtype != torch.int64 or index.dim() != 1:
            raise ValueError("RayBatcher.batch: a 1-D int64 index tensor expected")
        if index.device != self.device:
            raise ValueError("RayBatcher.batch: the index lives on %s, the batcher on %s" % (index.device, self.device))
        if self.rows is not None:
            index = self.rows[index]
        index = index.contiguous()
        if self.device.type != "cuda":
            return self._batch_host(index)
        from . import _lib
        n = int(index.numel())
        out = [torch.empty([n, 3], dtype=torch.float32, device=self.device) for _ in range(5 if self.with_index else 4)]
        with _lib.guard(self.device):
            _lib.check(_lib.load().ugrid_ray_batch(self.cams.data_ptr(), self.view_start.data_ptr(), self.n_views, index.data_ptr(), n,
                                                   self.images.data_ptr(), _STORES[self.store][1], int(self.inverse_y), int(self.flip_x),
                                                   int(self.flip_y), 1, int(self.ndc), 1.0, *[_lib.ptr(t) for t in out],
                                                   *([None] * (5 - len(out))), _lib.stream_of(index)), "ray_batch")
        return tuple(out) + (None,) * (5 - len(out))

    def _colour(self, index):
        rgb = self.images[index]
        return rgb if self.store == "float32" else (rgb.double() / 255.).to(torch.float32)

    def _batch_host(self, index):
        from .fourier_render import get_rays_of_pixel_index
        n = int(index.numel())
        view = torch.searchsorted(self.view_start, index, right=True) - 1       # the last view that starts at or before the pixel
        local = index - self.view_start[view]
        o, d, v = (torch.empty([n, 3], dtype=torch.float32) for _ in range(3))
        for vi in torch.unique(view).tolist():
            at = (view == vi).nonzero().flatten()
            H, W = self.HW[vi]
            r = get_rays_of_pixel_index(H, W, self.Ks[vi], self.poses[vi], local[at], inverse_y=self.inverse_y, flip_x=self.flip_x,
                                        flip_y=self.flip_y, ndc=self.ndc)
            o[at], d[at], v[at] = r
        idx = view.to(torch.float32)[:, None].expand(n, 3).contiguous() if self.with_index else None
        return self._colour(index), o, d, v, idx

    @torch.no_grad()
    def restrict(self, model, render_kwargs):
        """The 'in_maskcache' sampler (dvgo.py:619-657) without its table: view by view the view's rays exist transiently
        (get_rays_of_a_view), model.hit_coarse_geo marks the pixels whose rays meet the coarse geometry, and their global indices
        are appended to a device row list, so that batch(sel) afterwards means batch(rows[sel]).  Returns the per-view counts
        (the imsz of get_training_rays_in_maskcache_sampling; all zero, with an empty row list, when nothing survives)."""
        if self.ndc:
            raise NotImplementedError("NDC rays belong to the DirectMPIGO path, which has no mask-cache sampler")
        rows, imsz = [], []
        for vi, (H, W) in enumerate(self.HW):
            o, d, _ = get_rays_of_a_view(H, W, self.Ks[vi], self.poses[vi].to(self.device), inverse_y=self.inverse_y, flip_x=self.flip_x,
                                         flip_y=self.flip_y)
            mask = model.hit_coarse_geo(rays_o=o, rays_d=d, **render_kwargs).to(self.device)
            del o, d, _
            rows.append(mask.reshape(-1).nonzero().flatten() + int(self.view_start_host[vi]))
            imsz.append(int(rows[-1].numel()))
        self.rows = torch.cat(rows)
        return imsz


def device_batch_indices_generator(N, BS, device):
    """batch_indices_generator with the epoch's permutation resident on `device`: the same numpy draws, tail drop and redraw, ONE
    upload per epoch, and the batches are slices of it -- no per-iteration host-to-device copy."""
    device = torch.device(device)
    idx, top = torch.LongTensor(np.random.permutation(N)).to(device), 0
    while True:
        if top + BS > N:
            idx, top = torch.LongTensor(np.random.permutation(N)).to(device), 0
        yield idx[top:top + BS]
        top += BS


def gather_training_rays_lazy(model, data_dict, images, cfg, i_train, cfg_train, poses, HW, Ks, render_kwargs, device=None,
                              store="float32"):
    """gather_training_rays without the ray tables: the same dispatch (FourierGrid datasets carry the image index; then
    'in_maskcache' / 'flatten'; otherwise image-shaped views), returning (batcher, imsz, batch_index_sampler) for
    sample_batch_lazy.  The images and the pose table live on `device` whatever load2gpu_on_the_fly says: that is the point."""
    data = _get(cfg, 'data')
    if device is None:
        device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
    device = torch.device(device)
    rgb_tr_ori = [images[i] for i in i_train] if _get(data_dict, 'irregular_shape') else images[i_train]
    kw = dict(rgb_tr_ori=rgb_tr_ori, train_poses=poses[i_train], HW=HW[i_train], Ks=Ks[i_train], ndc=_get(data, 'ndc', False),
              inverse_y=_get(data, 'inverse_y', False), flip_x=_get(data, 'flip_x', False), flip_y=_get(data, 'flip_y', False),
              store=store, device=device)
    sampler = _get(cfg_train, 'ray_sampler')
    if _get(data, 'dataset_type') in FOURIERGRID_DATASETS or _get(cfg, 'model') == 'FourierGrid':
        batcher = RayBatcher.from_views(with_index=True, pos_emb=getattr(model, 'pos_emb', None), **kw)
        imsz = batcher.imsz
    elif sampler == 'in_maskcache':
        batcher = RayBatcher.from_views(with_index=False, **kw)
        imsz = batcher.restrict(model, render_kwargs)
    elif sampler == 'flatten':
        batcher = RayBatcher.from_views(with_index=False, **kw)
        imsz = batcher.imsz
    else:
        batcher = RayBatcher.from_views(with_index=False, image_shaped=True, **kw)
        imsz = batcher.imsz
    n_rows = len(batcher) if batcher.image_shape is None else batcher.n_views          # (len(rgb_tr) of gather_training_rays)
    index_generator = device_batch_indices_generator(n_rows, _get(cfg_train, 'N_rand'), device)
    return batcher, imsz, (lambda: next(index_generator))


def sample_batch_lazy(cfg_train, batcher, batch_index_sampler):
    """sample_batch on a RayBatcher: (target, rays_o, rays_d, viewdirs, indexs).  'flatten' / 'in_maskcache': the rows of
    batch_index_sampler(); 'random': the torch.randint calls of sample_batch in the same order on the batcher's device, so the
    generator state afterwards is the same -- three draws and the flat index b*H*W + r*W + c for image-shaped views, sel_b plus the
    ignored sel_r for flattened ones."""
    sampler = _get(cfg_train, 'ray_sampler')
    n_rand = _get(cfg_train, 'N_rand')
    dev = batcher.device
    if sampler in ('flatten', 'in_maskcache'):
        sel = batch_index_sampler()
        if sel.device != dev:
            sel = sel.to(dev, non_blocking=True)
    elif sampler == 'random':
        if batcher.image_shape is not None:
            N, H, W = batcher.image_shape
            sel_b, sel_r, sel_c = (torch.randint(k, [n_rand], device=dev) for k in (N, H, W))
            sel = sel_b * (H * W) + sel_r * W + sel_c
        else:
            sel = torch.randint(len(batcher), [n_rand], device=dev)
            torch.randint(3, [n_rand], device=dev)                                # (sample_batch's ignored sel_r)
    else:
        raise NotImplementedError(sampler)
    return batcher.batch(sel)


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
