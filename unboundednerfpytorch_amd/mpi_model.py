"""DirectMPIGO for TRAINING on the HIP ops: the counterpart of the reference's forward-facing model (dmpigo.py:18-340, the model
of every config with cfg.data.ndc -- configs/llff/*) with the same constructor arguments, the same parameter / buffer names
(`density.grid`, `k0.grid`, `act_shift.grid`, `rgbnet.*`, `viewfreq`, `mask_cache.*`, `xyz_min` / `xyz_max`: state_dicts and
`get_kwargs()` checkpoints interchange, also with mpi_render.mpi_state_from_reference_checkpoint) and the methods the training
program calls (`forward`, `scale_volume_grid`, `update_occupancy_cache`, `update_occupancy_cache_lt_nviews`, `sample_ray`,
`density_total_variation_add_grad`, `k0_total_variation_add_grad`, `activate_density`).

The training forward is FUSED like the other models': NDC sampling (every ray takes the same N_samples points), the box and
mask-cache tests, the density lookup PLUS the per-plane shift (act_shift, a [1,1,1,1,mpi_depth] grid whose lookup is a lerp
along z; the kernel reads the table from device memory, nothing is read back), Raw2Alpha with shift 0, both thresholds and
Alphas2Weights are one march + one compaction (grid.TrainSampleVox, cfg['mode'] == 'mpi'); llff's 3 x 64 rgbnet without view
frequencies runs on the fp32-MFMA kernels (ops.FusedRgbnet), and train_step.train_iteration's loss is ops.RenderLoss with
s = (step_id + 0.5) / N_samples.  `fused_forward = False` selects the op-by-op chain over the drop-in ops (the A/B twin of the
tests).  Inference should use mpi_render.DirectMPIGORenderer.  There is no CPU path: the ops raise without the HIP library.

With train_iteration's fused loss the fine stage (the default 3-layer rgbnet, every parameter trainable) takes the NATIVE step like
the other dense-grid models: native_step.VoxGOStep mode 'mpi' -- the same kernels on the same sizes in the same order as ONE autograd
node issued from C (ugrid_voxgo_step mode 3), the k0 update started between the two backward halves, and with `native_sync_free`
no host read at all, so the step can be captured in a hipGraph.  The per-plane shift is handed over as a device pointer and gets no
gradient; the samples' s come from the table sample_table() holds.  `native_step = False` keeps the four-node op-by-op step (the
tests' twin).  The coarse stage (no rgbnet) and non-default rgbnets stay on the op-by-op ops.

Not covered: data-parallel training."""
import numpy as np
import torch
import torch.nn.functional as F

from . import grid as _grid
from . import ops as _ops
from .train_model import make_rgbnet
from .voxgo_model import _VoxGOBase


class DirectMPIGO(_VoxGOBase):
    """The forward-facing model (dmpigo.py:18-340)."""
    native_step = True          # native_step.VoxGOStep mode 'mpi' (fine stage, train_iteration's fused loss); False: the op-by-op step
    fused_loss = True           # train_step.train_iteration: compositing + loss as ops.RenderLoss

    def __init__(self, xyz_min, xyz_max, num_voxels=0, mpi_depth=0, mask_cache_path=None, mask_cache_thres=1e-3,
                 mask_cache_world_size=None, fast_color_thres=0, density_type='DenseGrid', k0_type='DenseGrid', density_config={},
                 k0_config={}, rgbnet_dim=0, rgbnet_depth=3, rgbnet_width=128, viewbase_pe=0, **kwargs):
        super().__init__()
        backend = kwargs.get('backend')          # test hook, as FourierGridModel's: another implementation of the extension modules
        if backend is not None:
            self._be = backend
            self.fused_forward = self.fused_rgbnet = self.fused_loss = False
        self.register_buffer('xyz_min', torch.Tensor(xyz_min))
        self.register_buffer('xyz_max', torch.Tensor(xyz_max))
        self.fast_color_thres = fast_color_thres
        self._set_grid_resolution(num_voxels, mpi_depth)
        self.rgbnet_kwargs = {'rgbnet_dim': rgbnet_dim, 'rgbnet_depth': rgbnet_depth, 'rgbnet_width': rgbnet_width,
                              'viewbase_pe': viewbase_pe}
        if density_type != 'DenseGrid' or k0_type != 'DenseGrid':
            raise NotImplementedError("only DenseGrid (no config trains a TensoRF DirectMPIGO, and its per-axis TV differs)")
        # C = 9 (llff) is no multiple of 4: _make_grid keeps such a k0 in the canonical layout
        self._init_grids(density_type, k0_type, density_config, k0_config, 3 if rgbnet_dim <= 0 else rgbnet_dim,
                         backend is None and kwargs.get('channels_last_grids', True))
        # the density bias that makes the initial alpha of every sample on a ray equal (dmpigo.py:45-57): float64 recipe, one fp32
        # rounding per plane; not trained
        self.act_shift = _grid.FourierGrid(channels=1, world_size=[1, 1, mpi_depth], xyz_min=xyz_min, xyz_max=xyz_max,
                                           use_nerf_pos=False, fourier_freq_num=0)
        self.act_shift.query_fn = self._be.grid_query
        self.act_shift.grid.requires_grad = False
        with torch.no_grad():
            g = np.full([mpi_depth], 1. / mpi_depth - 1e-6)
            p = [1 - g[0]]
            for i in range(1, len(g)):
                p.append((1 - g[:i + 1].sum()) / (1 - g[:i].sum()))
            for i in range(len(p)):
                self.act_shift.grid[..., i].fill_(np.log(p[i] ** (-1 / self.voxel_size_ratio) - 1))
        if rgbnet_dim <= 0:
            self.rgbnet = None
        else:
            self.register_buffer('viewfreq', torch.FloatTensor([(2 ** i) for i in range(viewbase_pe)]))
            self.rgbnet = make_rgbnet(3 + 6 * viewbase_pe + self.k0_dim, rgbnet_width, rgbnet_depth)
        self.mask_cache_path, self.mask_cache_thres = mask_cache_path, mask_cache_thres
        if mask_cache_world_size is None:
            mask_cache_world_size = self.world_size
        if mask_cache_path:
            # the coarse stage's geometry at this model's mask vertices (dmpigo.py:104-113): a HIP lookup, like DirectVoxGO's
            if not torch.cuda.is_available():
                raise RuntimeError("mask_cache_path needs a HIP device (the mask-cache lookup has no CPU path)")
            dev = torch.device("cuda", torch.cuda.current_device())
            prior = _grid.MaskGrid(path=mask_cache_path, mask_cache_thres=mask_cache_thres).to(dev)
            mask = prior(self._vertices(mask_cache_world_size).to(dev)).cpu()
        else:
            mask = torch.ones([int(x) for x in mask_cache_world_size], dtype=torch.bool)
        self.mask_cache = self._new_mask(mask)

    def _set_grid_resolution(self, num_voxels, mpi_depth):
        """dmpigo.py:120-128: mpi_depth planes along z, x / y sized for num_voxels"""
        self.num_voxels = num_voxels
        self.mpi_depth = mpi_depth
        r = (num_voxels / self.mpi_depth / (self.xyz_max - self.xyz_min)[:2].prod()).sqrt()
        self.world_size = torch.zeros(3, dtype=torch.long)
        self.world_size[:2] = (self.xyz_max - self.xyz_min)[:2] * r
        self.world_size[2] = self.mpi_depth
        self.world_len = self.world_size[0].item()
        self.voxel_size_ratio = 256. / mpi_depth

    def get_kwargs(self):
        """`model_kwargs` of the reference's checkpoints (dmpigo.py:132-148)"""
        return {'xyz_min': self.xyz_min.cpu().numpy(), 'xyz_max': self.xyz_max.cpu().numpy(), 'num_voxels': self.num_voxels,
                'mpi_depth': self.mpi_depth, 'voxel_size_ratio': self.voxel_size_ratio, 'mask_cache_path': self.mask_cache_path,
                'mask_cache_thres': self.mask_cache_thres, 'mask_cache_world_size': list(self.mask_cache.mask.shape),
                'fast_color_thres': self.fast_color_thres, 'density_type': self.density_type, 'k0_type': self.k0_type,
                'density_config': self.density_config, 'k0_config': self.k0_config, **self.rgbnet_kwargs}

    # -- the pieces run_train.py calls -----------------------------------------------------------------------
    def activate_density(self, density, interval=None):
        """dmpigo.py:219-222: the shift is part of the density (act_shift is a grid), Raw2Alpha gets 0"""
        interval = interval if interval is not None else self.voxel_size_ratio
        return self._be.Raw2Alpha.apply(density.flatten(), 0, interval).reshape(density.shape)

    def tv_axis_weights(self, weight, which='density'):
        """dmpigo.py:209-217: x / y scaled by the larger of the two image-plane sizes, z by mpi_depth"""
        wxy = float(weight * self.world_size[:2].max() / 128)
        wz = float(weight * self.mpi_depth / 128)
        return (wxy, wxy, wz)

    def density_total_variation_add_grad(self, weight, dense_mode):
        self.density.total_variation_add_grad(*self.tv_axis_weights(weight, 'density'), dense_mode)

    def k0_total_variation_add_grad(self, weight, dense_mode):
        self.k0.total_variation_add_grad(*self.tv_axis_weights(weight, 'k0'), dense_mode)

    @torch.no_grad()
    def scale_volume_grid(self, num_voxels, mpi_depth):
        """Coarse-to-fine step (dmpigo.py:150-172): both grids resampled trilinearly, the mask cache rebuilt at the new resolution from
        the old cache and the 3x3x3 max-pooled alpha of density + act_shift.grid (the per-plane shift broadcast over x / y)."""
        self._set_grid_resolution(num_voxels, mpi_depth)
        self.density.scale_volume_grid(self.world_size)
        self.k0.scale_volume_grid(self.world_size)
        ws = self.world_size.tolist()
        if np.prod(ws) <= 256 ** 3:
            xyz = self._vertices(ws)
            dens = self.density.get_dense_grid() + self.act_shift.get_dense_grid()
            alpha = F.max_pool3d(self.activate_density(dens), kernel_size=3, padding=1, stride=1)[0, 0]
            self.mask_cache = self._new_mask(self.mask_cache(xyz) & (alpha > self.fast_color_thres)).to(xyz.device)
        self._hc_ver = None

    def update_occupancy_cache_lt_nviews(self, rays_o_tr, rays_d_tr, imsz, render_kwargs, maskout_lt_nviews):
        """mask &= (voxel seen by at least maskout_lt_nviews training views)  (dmpigo.py:189-207)"""
        dev = self.xyz_min.device
        count = torch.zeros(self.density.get_dense_grid().shape, dtype=torch.long, device=dev)
        for o_img, d_img in zip(rays_o_tr.split(imsz), rays_d_tr.split(imsz)):
            seen = torch.zeros([1, 1] + self.world_size.tolist(), device=dev).requires_grad_(True)      # (only its gradient is read)
            for o, d in zip(o_img.split(8192), d_img.split(8192)):
                pts = self.sample_ray(rays_o=o.to(dev), rays_d=d.to(dev), **render_kwargs)[0]
                (self._be.grid_query or _grid.GridQuery.apply)(seen, pts, self.xyz_min, self.xyz_max, 0).sum().backward()
            count += (seen.grad > 1)
        self.mask_cache.mask &= (count >= maskout_lt_nviews)[0, 0]

    def n_samples(self, stepsize):
        """samples per ray (dmpigo.py:239)"""
        return int((self.mpi_depth - 1) / stepsize) + 1

    def sample_table(self, stepsize, device):
        """train_iteration sizes the distortion term's interval (1 / n_max) from the sample table's length: N_samples entries,
        s = (j + 0.5) / N_samples as forward() returns it"""
        n = self.n_samples(stepsize)
        key = (n, str(device))
        cached = getattr(self, '_t_cache', None)
        if cached is not None and cached[0] == key:
            return cached[1]
        t = (torch.arange(n, dtype=torch.float32, device=device) + 0.5) / n
        self._t_cache = (key, t)
        return t

    def sample_ray(self, rays_o, rays_d, near, far, stepsize, **render_kwargs):
        """dmpigo.py:224-249: the in-box samples of every ray, near to far: pts [M,3], ray_id [M], step_id [M], N_samples"""
        assert near == 0 and far == 1
        ru = self._be.render_utils_cuda
        if ru is None:
            from . import render_utils_cuda as ru
        N_samples = self.n_samples(stepsize)
        pts, outbbox = ru.sample_ndc_pts_on_rays(rays_o.contiguous(), rays_d.contiguous(), self.xyz_min, self.xyz_max, N_samples)[:2]
        inb = ~outbbox
        dev = pts.device
        ray_id = torch.arange(inb.shape[0], device=dev).view(-1, 1).expand_as(inb)[inb]
        step_id = torch.arange(inb.shape[1], device=dev).view(1, -1).expand_as(inb)[inb]
        return pts[inb], ray_id, step_id, N_samples

    def _host_consts(self):
        """host copies of the mask cache's index map (the kernel takes it by value), refreshed only when it changes; the per-plane
        shift stays on the device"""
        mc = self.mask_cache
        ver = (mc.xyz2ijk_scale.data_ptr(), mc.xyz2ijk_scale._version, mc.xyz2ijk_shift._version, id(mc))
        if getattr(self, '_hc_ver', None) != ver:
            self._hc = {'mask_scale': mc.xyz2ijk_scale.tolist(), 'mask_shift': mc.xyz2ijk_shift.tolist()}
            self._hc_ver = ver
        return self._hc

    def forward(self, rays_o, rays_d, viewdirs, global_step=None, is_train=False, **render_kwargs):
        """Volume rendering of N NDC rays (dmpigo.py:251-340): the reference's return dict."""
        assert rays_o.dim() == 2 and rays_o.shape[-1] == 3, 'Only support point queries in [N, 3] format'
        N = rays_o.shape[0]
        dev = rays_o.device
        stepsize = render_kwargs['stepsize']
        interval = stepsize * self.voxel_size_ratio
        N_samples = self.n_samples(stepsize)
        density = None
        if self._can_fuse(rays_o):
            assert render_kwargs['near'] == 0 and render_kwargs['far'] == 1
            hc = self._host_consts()
            cfg = {'mode': 'mpi', 'interval': float(interval), 'thres': float(self.fast_color_thres), 'mask_scale': hc['mask_scale'],
                   'mask_shift': hc['mask_shift'], 'n_steps': N_samples, 'mpi_depth': int(self.mpi_depth),
                   'act_shift': self.act_shift.get_dense_grid().detach().reshape(-1)}
            fl = render_kwargs.get('fused_loss')
            native = self._native_params() if fl is not None else None
            if native is not None:
                # the whole step as one autograd node (native_step.VoxGOStep 'mpi'): the s table stands for (step_id + 0.5) / N_samples,
                # the nearclip term cannot apply (no raw density, no t in the reference's dict: its coefficient is zeroed, as below)
                coef = list(fl['coef'])
                coef[4] = coef[5] = 0.0
                bg = 'rand' if (render_kwargs.get('rand_bkgd', False) and global_step is not None) else render_kwargs['bg']
                out = self._native_forward(native, 'mpi', cfg, self.sample_table(stepsize, dev), rays_o.contiguous(), rays_d.contiguous(),
                                           viewdirs, {'target': fl['target'], 'coef': coef}, self._bg_rows(N, dev, bg, cached=True),
                                           self.mask_cache.mask)
                for k in ('raw_density', 'step_id'):       # (not in DirectMPIGO's return dict, dmpigo.py:320-340)
                    out.pop(k)
                out['s'] = out.pop('t')
                out['n_max'] = N_samples
                return out
            pts, density, alpha, weights, alphainv_last, ray_id, step_id, _, _ = _grid.TrainSampleVox.apply(
                self.density.grid, rays_o.contiguous(), rays_d.contiguous(), None, self.xyz_min, self.xyz_max, self.mask_cache.mask, cfg)
        else:
            if not rays_o.is_cuda and self._be.grid_query is None:
                raise RuntimeError("DirectMPIGO.forward has no CPU path: the rays must be on a HIP device")
            pts, ray_id, step_id, _ = self.sample_ray(rays_o=rays_o, rays_d=rays_d, **render_kwargs)
            if self.mask_cache is not None:
                m = self.mask_cache(pts)
                pts, ray_id, step_id = pts[m], ray_id[m], step_id[m]
            dens = self.density(pts) + self.act_shift(pts)
            alpha = self.activate_density(dens, interval)
            if self.fast_color_thres > 0:
                m = alpha > self.fast_color_thres
                pts, ray_id, step_id, alpha = pts[m], ray_id[m], step_id[m], alpha[m]
            weights, alphainv_last = self._be.Alphas2Weights.apply(alpha, ray_id, N)
            if self.fast_color_thres > 0:
                m = weights > self.fast_color_thres
                pts, ray_id, step_id, alpha, weights = pts[m], ray_id[m], step_id[m], alpha[m], weights[m]
        k0 = self.k0(pts)
        if k0.dim() == 1:
            k0 = k0.unsqueeze(-1)
        s = (step_id + 0.5) / N_samples         # int64 + 0.5 promotes to float32 (dmpigo.py:319)
        bg = 'rand' if (render_kwargs.get('rand_bkgd', False) and global_step is not None) else render_kwargs['bg']
        fused_loss = render_kwargs.get('fused_loss')
        if fused_loss is not None and density is not None:
            # the reference's DirectMPIGO returns no raw density and no t: the nearclip term cannot apply (its coefficient is zeroed)
            coef = list(fused_loss['coef'])
            coef[4] = coef[5] = 0.0
            logits = self._colour_logits(k0, viewdirs, ray_id)
            loss, mse, rgb_marched = self._render_loss({'target': fused_loss['target'], 'coef': coef}, logits, weights, alphainv_last,
                                                       density, ray_id, s, self._bg_rows(N, dev, bg), s=s)
            return {'alphainv_last': alphainv_last, 'weights': weights, 'rgb_marched': rgb_marched, 'raw_alpha': alpha,
                    'raw_logits': logits, 'ray_id': ray_id, 'n_max': N_samples, 's': s, 'loss': loss, 'mse': mse}
        rgb = torch.sigmoid(self._colour_logits(k0, viewdirs, ray_id))
        out = self._composed_tail(N, rgb, alpha, weights, alphainv_last, ray_id, step_id, bg, False)
        out.update(n_max=N_samples, s=s)
        if render_kwargs.get('render_depth', False):
            with torch.no_grad():
                out['depth'] = torch.zeros(N, device=dev).index_add_(0, ray_id, weights * s)
        return out
