"""TrainModel: what the three training models share -- voxgo_model.DirectVoxGO / DirectContractedVoxGO and
fourier_model.FourierGridModel, the counterparts of the reference's dvgo.py, dcvgo.py and FourierGrid_model.py.  One
definition each of: the rgbnet and its call, the grids and the mask cache with their hooks for an injected back-end, the
utilities the training program calls (activate_density, the two TV hooks, update_occupancy_cache, the mask rebuild of the
coarse-to-fine step, voxel_count_views), the sample-table cache of the contracted models, the admission rule and the call of
the native step (native_step.VoxGOStep), the background rows, and both training tails (ops.RenderLoss; the composed
index_add_ compositing).

A subclass supplies what differs: `_vertices` (each model keeps the reference's own arithmetic for the mask vertices), the
`*_density` / `*_rgb` resolution names, `table_end`, `_host_consts`, its sampling, and the keys of its return dict."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import grid as _grid
from . import ops as _ops

# the extension modules a model computes with: the HIP ops (None = the grid's / mask's own default, the HIP kernels)
HIP_BACKEND = SimpleNamespace(Raw2Alpha=_ops.Raw2Alpha, Alphas2Weights=_ops.Alphas2Weights, grid_query=None,
                              total_variation_cuda=None, render_utils_cuda=None)


def make_rgbnet(dim0, width, depth):
    net = nn.Sequential(nn.Linear(dim0, width), nn.ReLU(inplace=True),
                        *[nn.Sequential(nn.Linear(width, width), nn.ReLU(inplace=True)) for _ in range(depth - 2)],
                        nn.Linear(width, 3))
    nn.init.constant_(net[-1].bias, 0)
    return net


class TrainModel(nn.Module):
    _be = HIP_BACKEND           # FourierGridModel(backend=...): another implementation (the CPU oracle of the tests)
    fourier_freq_num = 0
    splitk_rgbnet = False       # ops.SplitKLinear weight gradients where ops.FusedRgbnet does not apply (FourierGridModel)
    table_end = None            # contracted models: the sample table's inner samples span [0, table_end]
    native_coarse = False       # True: the coarse stage (no rgbnet, 3-channel k0) of DirectVoxGO / DirectContractedVoxGO also takes
                                # native_step.VoxGOStep (colour 'none'); the other models ignore it
    _native_coarse_ok = False   # (the models whose forward passes the colour mode on)
    native_residual = False     # True: DirectVoxGO's residual-colour rgbnet (rgbnet_direct = False: rgbnet(k0[:, 3:], view) + k0[:, :3])
                                # also takes native_step.VoxGOStep (colour 'residual'); the other models ignore it
    _native_residual_ok = False
    fused_tensorf = False       # True: DirectVoxGO / DirectContractedVoxGO with a TensoRF density and / or k0 take the fused sampling too
                                # (grid.TrainSampleTensoRF over a factorised density, grid.TrainSampleVox over a dense one) and behind
                                # it the fused rgbnet and ops.RenderLoss; off until a measurement argues for it

    # -- construction helpers ------------------------------------------------------------------------------
    def _make_grid(self, channels, world_size, fourier, channels_last):
        # multi-channel grids are stored channel-last on the HIP ops (grid.FourierGrid: same logical parameter, one
        # 4C-byte run per voxel for the lookup / scatter / TV / Adam kernels); injected back-ends keep the canonical layout
        # (the channel-last TV / fused TV + Adam kernels index with 32 bits: a grid of >= 2^31 elements keeps the canonical
        # layout, whose kernels have a scalar 64-bit path -- ADVICE r2)
        n_levels = (1 + 2 * self.fourier_freq_num) if fourier else 1
        numel = n_levels * channels * int(world_size[0]) * int(world_size[1]) * int(world_size[2])
        cfg = {'channels_last': True} if (channels_last and channels > 1 and channels % 4 == 0 and numel < 2 ** 31) else None
        g = _grid.FourierGrid(channels=channels, world_size=world_size, xyz_min=self.xyz_min, xyz_max=self.xyz_max,
                              use_nerf_pos=fourier, fourier_freq_num=self.fourier_freq_num, config=cfg)
        g.query_fn, g.tv_module = self._be.grid_query, self._be.total_variation_cuda
        return g

    def _new_mask(self, mask):
        m = _grid.MaskGrid(path=None, mask=mask, xyz_min=self.xyz_min, xyz_max=self.xyz_max)
        m.lookup_module = self._be.render_utils_cuda
        return m

    # -- the pieces run_train.py calls -----------------------------------------------------------------------
    def activate_density(self, density, interval=None):
        interval = interval if interval is not None else self.voxel_size_ratio_density
        return self._be.Raw2Alpha.apply(density.flatten(), self.act_shift, interval).reshape(density.shape)

    def density_total_variation_add_grad(self, weight, dense_mode):
        w = weight * self.world_size_density.max() / 128
        self.density.total_variation_add_grad(w, w, w, dense_mode)

    def k0_total_variation_add_grad(self, weight, dense_mode):
        w = weight * self.world_size_rgb.max() / 128
        self.k0.total_variation_add_grad(w, w, w, dense_mode)

    def tv_axis_weights(self, weight, which='density'):
        """(wx, wy, wz) of a total-variation weight for the `which` ('density' / 'k0') grid: the model's own scaling of run_train.py's
        weight / batch size.  Here one number for all axes, world_size.max() / 128 (the two methods above); mpi_model.DirectMPIGO scales
        z by its plane count.  train_step.train_iteration hands the triple to the optimizer's TV pass."""
        w = float(weight * (self.world_size_density if which == 'density' else self.world_size_rgb).max() / 128)
        return (w, w, w)

    def _rebuild_mask_cache(self):
        """the mask half of the coarse-to-fine step (dvgo.py:227-234, dcvgo.py:167-174, FourierGrid_model.py:430-437): the cache
        rebuilt at the new density resolution from the old cache and the 3x3x3 max-pooled alpha (of level 0)"""
        ws = self.world_size_density.tolist()
        if np.prod(ws) <= 256 ** 3:
            xyz = self._vertices(ws)
            alpha = F.max_pool3d(self.activate_density(self.density.get_dense_grid()), kernel_size=3, padding=1, stride=1)[0, 0]
            self.mask_cache = self._new_mask(self.mask_cache(xyz) & (alpha > self.fast_color_thres)).to(xyz.device)

    @torch.no_grad()
    def update_occupancy_cache(self):
        """mask &= (3x3x3 max-pooled alpha at the cache's own vertices > fast_color_thres)  (dvgo.py:238-248, dcvgo.py:178-192,
        FourierGrid_model.py:440-453)"""
        xyz = self._vertices(self.mask_cache.mask.shape)
        alpha = self.activate_density(self.density(xyz)[None, None])
        alpha = F.max_pool3d(alpha, kernel_size=3, padding=1, stride=1)[0, 0]
        self.mask_cache.mask &= (alpha > self.fast_color_thres)

    def voxel_count_views(self, rays_o_tr, rays_d_tr, imsz, near, far, stepsize, downrate=1, irregular_shape=False):
        """How many training views see each voxel of a plain grid of the density resolution (dvgo.py:250-276,
        FourierGrid_model.py:392-418)"""
        from .train_rays import voxel_count_views
        return voxel_count_views(self._be.grid_query or _grid.GridQuery.apply, self.xyz_min, self.xyz_max, self.voxel_size_density,
                                 self.world_size_density, self._density_grid_shape(), rays_o_tr, rays_d_tr, imsz, near,
                                 stepsize, downrate, irregular_shape)

    def _has_tensorf(self, *grids):
        """is one of `grids` (default: density and k0) a TensoRF grid?  Such a model takes the composed forward unless `fused_tensorf`
        asks for the fused sampling; there is no native step over factorised grids"""
        grids = grids or (getattr(self, 'density', None), getattr(self, 'k0', None))
        return any(isinstance(g, _grid.TensoRFGrid) for g in grids)

    def _density_grid_shape(self):
        """the shape of the dense density grid -- read off the world size for a TensoRF density (no bake just for a shape)"""
        if self._has_tensorf(self.density):
            return torch.Size([1, 1] + [int(x) for x in self.world_size_density])
        return self.density.get_dense_grid().shape

    # -- the contracted models' sample table -------------------------------------------------------------------
    def _sample_table(self, stepsize):
        """the mid-point sample distances of sample_ray (dcvgo.py:243-250, FourierGrid_model.py:524-531), [S] on the host"""
        n_inner = int(2 / (2 + 2 * self.bg_len) * self.world_len_density / stepsize) + 1
        b_inner = torch.linspace(0, self.table_end, n_inner + 1)
        b_outer = self.table_end / torch.linspace(1, 1 / 128, n_inner + 1)
        return torch.cat([(b_inner[1:] + b_inner[:-1]) * 0.5, (b_outer[1:] + b_outer[:-1]) * 0.5])

    def sample_table(self, stepsize, device):
        key = (float(stepsize), int(self.world_len_density), str(device))
        cached = getattr(self, '_t_cache', None)
        if cached is not None and cached[0] == key:
            return cached[1]
        t = self._sample_table(stepsize).to(device)
        self._t_cache = (key, t)
        return t

    # -- the native step ---------------------------------------------------------------------------------------
    def _can_fuse(self, rays_o):
        """the fused sampling ops need fast_color_thres > 0, like the reference's own masking branches; a model with a TensoRF grid
        takes them only where `fused_tensorf` asks for it, and a TensoRF density only while the HIP lookup is its lookup (the march
        computes tf_density: an injected query function would not be what it samples)"""
        if not (self.fused_forward and self.fast_color_thres > 0 and rays_o.is_cuda):
            return False
        if not self._has_tensorf():
            return True
        return self.fused_tensorf and not (self._has_tensorf(self.density) and self.density.query_fn is not None)

    def _fused_sample(self, rays_o, rays_d, t, cfg):
        """the fused sampling op of this model's density type: the nine outputs of grid.TrainSampleVox"""
        o, d = rays_o.contiguous(), rays_d.contiguous()
        if self._has_tensorf(self.density):
            return _grid.TrainSampleTensoRF.apply(*self.density.factors(), o, d, t, self.xyz_min, self.xyz_max, self.mask_cache.mask, cfg)
        return _grid.TrainSampleVox.apply(self.density.grid, o, d, t, self.xyz_min, self.xyz_max, self.mask_cache.mask, cfg)

    def _native_params(self):
        """The parameters of native_step.VoxGOStep (density grid, k0 grid, the rgbnet's three weights and biases), or None when this
        configuration takes the op-by-op ops: the native step needs the default 3-layer rgbnet fed by all of k0 (rgbnet_direct, where
        the model has the choice), gradients on, every one of those parameters trainable, and both grids looked up by the HIP kernels
        (no injected query function) with the levels they were built with.
        The coarse stage -- no rgbnet, the colour is the 3-channel k0 itself -- takes the native step only where `native_coarse` asks
        for it: the two grids followed by six None (VoxGOStep colour 'none').  The residual-colour rgbnet (rgbnet_direct = False) takes it
        only where `native_residual` asks for it, under the conditions of the direct one plus a k0 of >= 4 channels (colour 'residual')."""
        if not (self.native_step and torch.is_grad_enabled()) or self._has_tensorf():
            return None
        if self.rgbnet is None:
            if not (self.native_coarse and self._native_coarse_ok and self.k0.grid.shape[1] == 3):
                return None
            nets = [None] * 6
        else:
            if not self.fused_rgbnet:
                return None
            if self._residual_colour() and not (self.native_residual and self._native_residual_ok and self.k0.grid.shape[1] >= 4):
                return None
            lin = _ops.rgbnet_linears(self.rgbnet)
            if lin is None:
                return None
            nets = [p for l in lin for p in (l.weight, l.bias)]
        params = [self.density.grid, self.k0.grid] + nets
        if not all(p.requires_grad for p in params if p is not None) \
                or any(g.query_fn is not None or g.grid.shape[0] != 1 + 2 * max(g.nerf_pos_num_freq, 0) for g in (self.density, self.k0)):
            return None
        return params

    def _residual_colour(self):
        """the rgbnet sees k0[:, 3:] and its output is added to k0[:, :3] (DirectVoxGO with rgbnet_direct = False)"""
        return self.rgbnet is not None and not getattr(self, 'rgbnet_direct', True)

    def _native_forward(self, params, mode, cfg, t, rays_o, rays_d, viewdirs, fused_loss, bg, mask):
        """The training forward + loss as ONE autograd node issued from C (native_step.VoxGOStep): the same kernels, sizes and order
        as the op-by-op ops; the reference's return dict with loss / mse added, the per-sample arrays detached"""
        from .native_step import VoxGOStep
        pack = {'mode': mode, 'cfg': cfg, 't': t, 'rays_o': rays_o, 'rays_d': rays_d, 'viewdirs': viewdirs,
                'viewfreq': self.viewfreq if self.rgbnet is not None else None, 'colour': 'none' if self.rgbnet is None else 'residual' if self._residual_colour() else 'rgbnet',
                'xyz_min': self.xyz_min, 'xyz_max': self.xyz_max, 'k0_xyz_min': self.k0.xyz_min, 'k0_xyz_max': self.k0.xyz_max,
                'mask': mask, 'target': fused_loss['target'], 'bg': bg, 'coef': fused_loss['coef'], 'sync_free': self.native_sync_free}
        loss, mse = VoxGOStep.apply(*params, pack)
        o = pack['out']
        return {'alphainv_last': o['alphainv_last'], 'weights': o['weights'], 'rgb_marched': o['rgb_marched'], 'raw_alpha': o['raw_alpha'],
                'raw_density': o['raw_density'], 'raw_logits': o['raw_logits'], 'ray_id': o['ray_id'], 'step_id': o['step_id'],
                't': o['t'], 'loss': loss, 'mse': mse, 'loss_mse': o['loss_mse'], 'native': pack}

    def _bg_rows(self, N, dev, bg, cached=False):
        """The fused loss's background colour as [N,3] rows.  bg: 'rand' (ONE uniform draw), a constant or None (none / black: no
        rows) -- `cached`: read-only constant rows kept between steps (one fill launch less per iteration, the native step), else a
        fresh fill (the op-by-op tail)"""
        if isinstance(bg, str):
            return torch.rand(N, 3, device=dev)
        if bg is None or float(bg) == 0.0:
            return None
        if not cached:
            return torch.full((N, 3), float(bg), device=dev)
        key = (int(N), float(bg), str(dev))
        kept = getattr(self, '_bg_kept', None)
        if kept is None or kept[0] != key:
            kept = (key, torch.full((N, 3), float(bg), device=dev))
            object.__setattr__(self, '_bg_kept', kept)
        return kept[1]

    # -- colour and the two training tails ---------------------------------------------------------------------
    def _logits(self, k0_view, viewdirs, ray_id):
        """rgbnet([k0, view embedding]) of the surviving samples (FourierGrid_model.py:631-636).  While training the default 3-layer
        net runs on the hand-written fp32-MFMA kernels (ops.FusedRgbnet: no library GEMMs; the embedding rows are formed inside,
        with the concatenation); other networks take torch's layers, with ops.SplitKLinear weight gradients when splitk_rgbnet"""
        train = k0_view.is_cuda and torch.is_grad_enabled()
        lin = _ops.rgbnet_linears(self.rgbnet) if (self.fused_rgbnet and train) else None
        if lin is not None:
            rows = _ops.ViewRows(viewdirs, self.viewfreq, ray_id)
            return _ops.FusedRgbnet.apply(k0_view, rows, lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias, lin[2].weight, lin[2].bias)
        feat = torch.cat([k0_view, _ops.rgbnet_features(None, viewdirs, self.viewfreq, ray_id)], -1)
        if self.splitk_rgbnet and train:
            return _ops.sequential_splitk(self.rgbnet, feat)
        return self.rgbnet(feat)

    def _colour_logits(self, k0, viewdirs, ray_id, residual=False):
        """The colour logits of the surviving samples (dvgo.py:377-398, dcvgo.py:332-344): the rgbnet's output (+ the diffuse channels
        of the residual model) or, in the coarse stage, the 3-channel k0 itself; rgb = sigmoid of them"""
        if self.rgbnet is None:
            return k0
        if residual:
            return self._logits(k0[:, 3:].contiguous(), viewdirs, ray_id) + k0[:, :3]
        return self._logits(k0, viewdirs, ray_id)

    def _render_loss(self, fused_loss, logits, weights, alphainv_last, density, ray_id, tt, bg, s=None):
        """Training tail as ONE op (ops.RenderLoss): sigmoid, compositing, background and the loss terms of run_train.py:254-279.
        train_step.train_iteration passes fused_loss = {'target': [N,3], 'coef': ops.loss_coefficients(...)}.
        s: the samples' normalised distances where they are not 1 - 1 / (1 + t) (DirectMPIGO).  -> loss, mse, rgb_marched"""
        return _ops.RenderLoss.apply(logits.contiguous(), weights, alphainv_last, density, ray_id, tt, s, fused_loss['target'], bg,
                                     fused_loss['coef'])

    def _composed_tail(self, N, rgb, alpha, weights, alphainv_last, ray_id, step_id, bg, render_depth, contracted=None):
        """The reference's tail op by op (dvgo.py:400-424, dcvgo.py:346-383, FourierGrid_model.py:638-671): index_add_ compositing,
        the background -- bg as _bg_rows takes it, the draw coming after the compositing -- and the return dict.
        contracted = (raw density, n_max, t) of the samples: the contracted models' keys, s = 1 - 1/(1+t) and depth from s; the
        bounded model's depth is from step_id."""
        dev = weights.device
        rgb_marched = torch.zeros(N, 3, device=dev).index_add_(0, ray_id, weights.unsqueeze(-1) * rgb)
        if isinstance(bg, str):
            bg = torch.rand_like(rgb_marched)
        if bg is not None:
            rgb_marched = rgb_marched + alphainv_last.unsqueeze(-1) * bg
        out = {'alphainv_last': alphainv_last, 'weights': weights, 'rgb_marched': rgb_marched, 'raw_alpha': alpha, 'raw_rgb': rgb,
               'ray_id': ray_id}
        depth_of = step_id
        if contracted is not None:
            density, n_max, tt = contracted
            depth_of = s = 1 - 1 / (1 + tt)
            out.update(raw_density=density, step_id=step_id, n_max=n_max, t=tt, s=s)
        if render_depth:
            with torch.no_grad():
                out['depth'] = torch.zeros(N, device=dev).index_add_(0, ray_id, weights * depth_of)
        return out
