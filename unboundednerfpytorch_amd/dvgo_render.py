"""DirectVoxGORenderer: inference forward of the reference's bounded model dvgo.DirectVoxGO
(/root/reference/FourierGrid/dvgo.py:306-425, BASELINE.json configs[0]) composed from the drop-in kernels:
sample_pts_on_rays (ray-AABB clip + variable-length marching) -> maskcache_lookup -> dense grid query ->
raw2alpha -> alpha2weight -> k0 query -> rgbnet -> per-ray sums.  Same call signature and return keys as the
reference forward (`rgb_marched`, `depth`, `alphainv_last`, `weights`, `raw_alpha`, `raw_rgb`, `ray_id`).

The compaction steps (boolean masks) and the tiny rgbnet use torch on the device, exactly like the
reference does; every kernel the reference has natively is the HIP one.

Also the training-ray preparation that leans on the same kernels: `hit_coarse_geo`
(dvgo.py:292-304) and `voxel_count_views` (dvgo.py:247-277), both one-line calls of train_rays' functions of those names, and `get_training_rays_in_maskcache_sampling`
(dvgo.py:619-657).  `ops` / `query` / `grad_query` exist for tests: they let the same composition run against another
implementation of the extension modules (the CPU oracle); the default is the HIP library, which needs a GPU.
"""
import torch

from .bounded_render import BoundedRenderer


def dvgo_state_from_params(xyz_min, xyz_max, num_voxels, num_voxels_base, alpha_init, density_grid, k0_grid, rgbnet_weights,
                           rgbnet_biases, mask, fast_color_thres, rgbnet_direct, viewbase_pe=4):
    """The renderer's `state` from DirectVoxGO's constructor arguments and learned tensors: voxel sizes and world size as
    __init__ / _set_grid_resolution derive them (dvgo.py:40-56, 154-163), act_shift = log(1/(1-alpha_init) - 1) (:49), the
    world -> mask index map of its MaskGrid (grid.py:221-228).  All fp32 tensor arithmetic, like the reference."""
    import math
    lo, hi = torch.Tensor(xyz_min), torch.Tensor(xyz_max)
    vol = (hi - lo).prod()
    voxel_size = (vol / num_voxels).pow(1 / 3)
    scale = (torch.Tensor(list(mask.shape)) - 1) / (hi - lo)
    return {'xyz_min': lo, 'xyz_max': hi, 'voxel_size': voxel_size, 'voxel_size_ratio': voxel_size / (vol / num_voxels_base).pow(1 / 3),
            'world_size': ((hi - lo) / voxel_size).long(), 'act_shift': torch.FloatTensor([math.log(1 / (1 - alpha_init) - 1)]),
            'density_grid': density_grid, 'k0_grid': k0_grid, 'rgbnet_weights': list(rgbnet_weights),
            'rgbnet_biases': list(rgbnet_biases), 'mask': mask.bool(), 'xyz2ijk_scale': scale, 'xyz2ijk_shift': -lo * scale,
            'fast_color_thres': fast_color_thres, 'rgbnet_direct': bool(rgbnet_direct), 'viewbase_pe': int(viewbase_pe)}


def dvgo_state_from_reference_checkpoint(ckpt):
    """`state` from a checkpoint the reference's trainer wrote for a DirectVoxGO model ({'model_kwargs', 'model_state_dict'},
    run_train.py / utils.load_model): dense grids only (density_type = k0_type = 'DenseGrid', the default)."""
    kw, sd = ckpt['model_kwargs'], ckpt['model_state_dict']
    if kw.get('density_type', 'DenseGrid') != 'DenseGrid' or kw.get('k0_type', 'DenseGrid') != 'DenseGrid':
        raise NotImplementedError("only DenseGrid checkpoints (TensoRFGrid is outside the hot path, SURVEY.md section 8)")
    if kw.get('rgbnet_full_implicit', False):
        raise NotImplementedError("rgbnet_full_implicit models have no feature grid")
    lin = sorted({k[:-len('.weight')] for k in sd if k.startswith('rgbnet.') and k.endswith('.weight')},
                 key=lambda n: [int(x) for x in n.split('.')[1:]])
    st = dvgo_state_from_params(
        [float(x) for x in kw['xyz_min']], [float(x) for x in kw['xyz_max']], kw['num_voxels'], kw['num_voxels_base'], kw['alpha_init'], sd['density.grid'], sd['k0.grid'],
        [sd[n + '.weight'] for n in lin], [sd[n + '.bias'] for n in lin], sd['mask_cache.mask'], kw.get('fast_color_thres', 0),
        kw.get('rgbnet_direct', False), kw.get('viewbase_pe', 4))
    for k in ('xyz2ijk_scale', 'xyz2ijk_shift'):          # the stored buffers win over the re-derived ones
        if 'mask_cache.' + k in sd:
            st[k] = sd['mask_cache.' + k]
    return st


def dvgo_state_from_tensorf_checkpoint(ckpt, device, mem_get_info=None):
    """`state` from a DirectVoxGO checkpoint whose density and / or k0 is a TensoRFGrid (configs/nerf/ship.tensorf.py): the TensoRF
    grids baked on `device` (bounded_render.bake_tensorf_checkpoint: exact, memory-checked), then dvgo_state_from_reference_checkpoint"""
    from .bounded_render import bake_tensorf_checkpoint, stored_buffers_win
    return stored_buffers_win(dvgo_state_from_reference_checkpoint(bake_tensorf_checkpoint(ckpt, device, mem_get_info)), ckpt, ('act_shift',))


class DirectVoxGORenderer(BoundedRenderer):
    """state: xyz_min/xyz_max [3], density_grid [1,1,X,Y,Z], k0_grid [1,C,X,Y,Z], rgbnet_weights/biases (lists),
    mask [mx,my,mz] bool, xyz2ijk_scale/shift [3], act_shift, voxel_size, voxel_size_ratio (0-d tensors or floats),
    fast_color_thres, rgbnet_direct, viewbase_pe.

    render_rays: the whole chain of dvgo.py:306-425 in two launches.  The reference (and forward()) size the sample list by a
    count kernel, a cumsum and a HOST READ of the total before the fill (render_utils_kernel.cu:100-260, `.item()` in
    sample_pts_on_rays); in the fused march a lane marches its ray to the ray's own step count, so nothing is read back.
    render_kwargs as forward(): near, stepsize, bg, render_depth, plus FourierGridRenderer's ray_order."""

    @classmethod
    def from_reference_checkpoint(cls, ckpt, device):
        """ckpt: the dict the reference saves for a DirectVoxGO model (torch.load('fine_last.tar', weights_only=False))"""
        return cls(dvgo_state_from_reference_checkpoint(ckpt), device)

    @classmethod
    def from_tensorf_checkpoint(cls, ckpt, device, mem_get_info=None):
        """ckpt: a DirectVoxGO checkpoint with TensoRF grids; they are baked once on `device`, the fused kernels render the result"""
        return cls(dvgo_state_from_tensorf_checkpoint(ckpt, device, mem_get_info), device)

    # -- fused inference path ----------------------------------------------------------------------------------
    @property
    def rgbnet_residual(self):
        """the diffuse + residual colour of dvgo.py:385-398: rgbnet on [k0[3:], embedding], k0[:3] added to its output"""
        return len(self.s['rgbnet_weights']) > 0 and not bool(self.s['rgbnet_direct'])

    def fused_supported(self):
        """the fused march (ugrid_render_march_dvgo) + shade kernels cover what BoundedRenderer.fused_supported lists, the
        rgbnet being the DIRECT 3 x 128 one on [k0 (12), view embedding] -- rgbnet_direct -- or the residual one: the network
        reads channels 3.. and the first three are added to its output -- the shade kernels' residual epilogue
        (include/ugrid_hip.h: UGRID_MLP_RESIDUAL), C >= 9"""
        return super().fused_supported() and (not self.rgbnet_residual or int(self.s['k0_grid'].shape[1]) >= 9)

    frames_in_flight = 4      # run_render.render_viewpoints: a bounded scene's view (800 x 800 on the lego box: two launches of ~0.9 ms that leave most of
                              # the chip idle) gains from four views in flight -- 1.88 / 1.03 / 0.78 ms per view at 1 / 2 / 4 (profiles/r06/frames_in_flight_sweep.txt)

    def _fused_state(self):
        st = self._bounded_state('dvgo', {'voxel_size': self.s['voxel_size']})
        st.update(act_shift=float(self.s['act_shift']), rgbnet_residual=self.rgbnet_residual)
        return st

    @torch.no_grad()
    def forward(self, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        s = self.s
        assert rays_o.dim() == 2 and rays_o.shape[-1] == 3, 'Only suuport point queries in [N, 3] format'
        N = rays_o.shape[0]
        stepsize = render_kwargs['stepsize']
        far = 1e9  # the given far can be too small while rays stop when hitting scene bbox (dvgo.py:318)
        stepdist = stepsize * s['voxel_size']
        ray_pts, mask_outbbox, ray_id, step_id = self.ru.sample_pts_on_rays(
            rays_o.contiguous(), rays_d.contiguous(), s['xyz_min'], s['xyz_max'], render_kwargs['near'], far, stepdist)[:4]
        inb = ~mask_outbbox
        ray_pts, ray_id, step_id = ray_pts[inb], ray_id[inb], step_id[inb]
        interval = stepsize * s['voxel_size_ratio']
        m = self.ru.maskcache_lookup(s['mask'], ray_pts.contiguous(), s['xyz2ijk_scale'], s['xyz2ijk_shift'])
        ray_pts, ray_id, step_id = ray_pts[m], ray_id[m], step_id[m]
        density = self.query(s['density_grid'], ray_pts, s['xyz_min'], s['xyz_max'], 0)
        alpha = self.ru.raw2alpha(density.flatten().contiguous(), s['act_shift'], interval)[1]
        thres = float(s['fast_color_thres'])
        if thres > 0:
            k = alpha > thres
            ray_pts, ray_id, step_id, alpha = ray_pts[k], ray_id[k], step_id[k], alpha[k]
        weights, _, alphainv_last = self.ru.alpha2weight(alpha.contiguous(), ray_id.contiguous(), N)[:3]
        if thres > 0:
            k = weights > thres
            weights, alpha, ray_pts, ray_id, step_id = weights[k], alpha[k], ray_pts[k], ray_id[k], step_id[k]
        rgb, rgb_marched = self._colour(ray_pts, ray_id, weights, alphainv_last, viewdirs, N, render_kwargs['bg'])
        out = {'alphainv_last': alphainv_last, 'weights': weights, 'rgb_marched': rgb_marched, 'raw_alpha': alpha,
               'raw_rgb': rgb, 'ray_id': ray_id}
        if render_kwargs.get('render_depth', False):
            out['depth'] = torch.zeros(N, device=rays_o.device).index_add_(0, ray_id, weights * step_id)
        return out

    __call__ = forward

    # -- training-ray preparation ---------------------------------------------------------------------------
    def hit_coarse_geo(self, rays_o, rays_d, near, far, stepsize, **render_kwargs):
        """bool [...]: does the ray pass through a cell the mask cache marks as possibly occupied? (dvgo.py:292-304)"""
        from .train_rays import hit_coarse_geo
        s = self.s
        return hit_coarse_geo(self.ru, rays_o, rays_d, s['xyz_min'], s['xyz_max'], near, stepsize * s['voxel_size'], s['mask'],
                              s['xyz2ijk_scale'], s['xyz2ijk_shift'])

    def voxel_count_views(self, rays_o_tr, rays_d_tr, imsz, near, far, stepsize, downrate=1, irregular_shape=False):
        """Per-voxel count of the training views that see it (dvgo.py:247-277), scattered by self.grad_query's backward"""
        from .train_rays import voxel_count_views
        s = self.s
        return voxel_count_views(self.grad_query, s['xyz_min'], s['xyz_max'], s['voxel_size'], s['world_size'], s['density_grid'].shape,
                                 rays_o_tr, rays_d_tr, imsz, near, stepsize, downrate, irregular_shape)


@torch.no_grad()
def get_training_rays_in_maskcache_sampling(rgb_tr_ori, train_poses, HW, Ks, ndc, inverse_y, flip_x, flip_y, model,
                                            render_kwargs, get_rays=None):
    """Keep only the pixels whose rays hit the coarse geometry (dvgo.py:619-657); returns the flattened
    (rgb, rays_o, rays_d, viewdirs, imsz).  model: DirectVoxGORenderer (anything with hit_coarse_geo)."""
    assert len(rgb_tr_ori) == len(train_poses) and len(rgb_tr_ori) == len(Ks) and len(rgb_tr_ori) == len(HW)
    if ndc:
        raise NotImplementedError("NDC rays belong to the DirectMPIGO path (out of scope, SURVEY.md section 2)")
    if get_rays is None:
        from .fourier_render import get_rays_of_a_view as get_rays
    dev = rgb_tr_ori[0].device
    total = sum(im.shape[0] * im.shape[1] for im in rgb_tr_ori)
    rgb_tr = torch.zeros(total, 3, device=dev)
    rays_o_tr, rays_d_tr, viewdirs_tr = torch.zeros_like(rgb_tr), torch.zeros_like(rgb_tr), torch.zeros_like(rgb_tr)
    imsz, top = [], 0
    for c2w, img, (H, W), K in zip(train_poses, rgb_tr_ori, HW, Ks):
        assert img.shape[:2] == (H, W)
        rays_o, rays_d, viewdirs = get_rays(H, W, K, torch.as_tensor(c2w, dtype=torch.float32).to(dev),
                                            inverse_y=inverse_y, flip_x=flip_x, flip_y=flip_y)
        mask = model.hit_coarse_geo(rays_o=rays_o, rays_d=rays_d, **render_kwargs).to(dev)   # whole image at once
        n = int(mask.sum())
        rgb_tr[top:top + n] = img[mask]
        rays_o_tr[top:top + n] = rays_o[mask]
        rays_d_tr[top:top + n] = rays_d[mask]
        viewdirs_tr[top:top + n] = viewdirs[mask]
        imsz.append(n)
        top += n
    return rgb_tr[:top], rays_o_tr[:top], rays_d_tr[:top], viewdirs_tr[:top], imsz
