"""DirectMPIGORenderer: inference forward of the reference's forward-facing model dmpigo.DirectMPIGO
(/root/reference/FourierGrid/dmpigo.py:224-338; the model run_render.py / run_train.py pick when cfg.data.ndc is set, e.g.
configs/llff/*.py).  NDC rays, a fixed number of samples per ray, a dense density grid plus a per-plane shift
(act_shift, a [1,1,1,1,mpi_depth] DenseGrid), the mask cache, Raw2Alpha / Alphas2Weights and either sigmoid(k0) or the
rgbnet on [k0, view embedding].

Two paths with the same outputs:
  forward      the composition of the drop-in kernels (sample_ndc_pts_on_rays -> maskcache_lookup -> grid query + act_shift
               -> raw2alpha -> alpha2weight -> k0 query -> rgbnet -> per-ray sums), like the reference; `ops` / `query` let
               the same code run over another implementation of the extension modules (the CPU oracle in tests).
  render_rays  the fused march (ugrid_render_march_mpi) + shade kernels through FourierGridRenderer's `mpi` variant.
"""
import torch

from .bounded_render import BoundedRenderer


def mpi_state_from_params(xyz_min, xyz_max, num_voxels, mpi_depth, density_grid, act_shift_grid, k0_grid, rgbnet_weights,
                          rgbnet_biases, mask, fast_color_thres, viewbase_pe=0):
    """The renderer's `state` from DirectMPIGO's constructor arguments and learned tensors: world size and voxel_size_ratio as
    _set_grid_resolution derives them (dmpigo.py:120-130), the world -> mask index map of its MaskGrid (grid.py:221-228)."""
    lo, hi = torch.Tensor(xyz_min), torch.Tensor(xyz_max)
    r = (num_voxels / mpi_depth / (hi - lo)[:2].prod()).sqrt()
    world_size = torch.zeros(3, dtype=torch.long)
    world_size[:2] = (hi - lo)[:2] * r
    world_size[2] = mpi_depth
    scale = (torch.Tensor(list(mask.shape)) - 1) / (hi - lo)
    return {'xyz_min': lo, 'xyz_max': hi, 'world_size': world_size, 'mpi_depth': int(mpi_depth),
            'voxel_size_ratio': 256. / mpi_depth, 'density_grid': density_grid, 'act_shift': act_shift_grid, 'k0_grid': k0_grid,
            'rgbnet_weights': list(rgbnet_weights), 'rgbnet_biases': list(rgbnet_biases), 'mask': mask.bool(),
            'xyz2ijk_scale': scale, 'xyz2ijk_shift': -lo * scale, 'fast_color_thres': fast_color_thres,
            'viewbase_pe': int(viewbase_pe)}


def mpi_state_from_reference_checkpoint(ckpt):
    """`state` from a checkpoint the reference's trainer wrote for a DirectMPIGO model ({'model_kwargs', 'model_state_dict'}:
    get_kwargs() / state_dict(), dmpigo.py:132-148): dense grids only (density_type = k0_type = 'DenseGrid', the default)."""
    kw, sd = ckpt['model_kwargs'], ckpt['model_state_dict']
    if kw.get('density_type', 'DenseGrid') != 'DenseGrid' or kw.get('k0_type', 'DenseGrid') != 'DenseGrid':
        raise NotImplementedError("only DenseGrid checkpoints (TensoRFGrid is outside the hot path, SURVEY.md section 8)")
    lin = sorted({k[:-len('.weight')] for k in sd if k.startswith('rgbnet.') and k.endswith('.weight')},
                 key=lambda n: [int(x) for x in n.split('.')[1:]])
    st = mpi_state_from_params(
        [float(x) for x in kw['xyz_min']], [float(x) for x in kw['xyz_max']], kw['num_voxels'], kw['mpi_depth'], sd['density.grid'],
        sd['act_shift.grid'], sd['k0.grid'], [sd[n + '.weight'] for n in lin], [sd[n + '.bias'] for n in lin], sd['mask_cache.mask'],
        kw.get('fast_color_thres', 0), kw.get('viewbase_pe', 0))
    for k in ('xyz2ijk_scale', 'xyz2ijk_shift'):          # the stored buffers win over the re-derived ones
        if 'mask_cache.' + k in sd:
            st[k] = sd['mask_cache.' + k]
    return st


class DirectMPIGORenderer(BoundedRenderer):
    """state: xyz_min/xyz_max [3] (the NDC box), density_grid [1,1,X,Y,D], act_shift [1,1,1,1,D], k0_grid [1,C,X,Y,D],
    rgbnet_weights/biases (lists; empty: rgb = sigmoid(k0), C = 3), mask [mx,my,mz] bool, xyz2ijk_scale/shift [3],
    mpi_depth = D, voxel_size_ratio = 256 / D, fast_color_thres, viewbase_pe.

    render_rays: the whole chain of dmpigo.py:224-338 in two launches.  NDC rays (rays_o / rays_d from
    get_rays_of_a_view(ndc=True)), world viewdirs; render_kwargs as forward(): near (0), far (1), stepsize, bg, render_depth,
    plus FourierGridRenderer's ray_order."""

    ndc = True
    ray_order = "coherent"
    # render_view: NDC rays generated on the device in 8 x 8 pixel blocks (fourier_render.render_view_of, ndc=True).  A view whose
    # sides are not multiples of 8 (LLFF's 1008 x 756) is rendered in image order, which is coherent too: 64 consecutive pixels
    # of a row.  (The "auto" check of FourierGridRenderer would sort such a list: NDC origins move across the image with the pixel.)

    def __init__(self, state, device, ops=None, query=None, mlp_mode=None):
        super().__init__(state, device, ops, query, mlp_mode=mlp_mode)

    @classmethod
    def from_reference_checkpoint(cls, ckpt, device, **kw):
        """ckpt: the dict the reference saves for a DirectMPIGO model (torch.load('fine_last.tar', weights_only=False))"""
        return cls(mpi_state_from_reference_checkpoint(ckpt), device, **kw)

    def n_samples(self, stepsize):
        """samples per ray, int((mpi_depth - 1) / stepsize) + 1 (dmpigo.py:241)"""
        return int((int(self.s['mpi_depth']) - 1) / stepsize) + 1

    def act_shift_at(self, pts):
        """act_shift(pts): grid_sample(align_corners=True) of the [1,1,1,1,D] grid -- its one-voxel x / y axes map to index 0
        with weight 1, so the value is the lerp along z, formed as grid_sample forms it (v0 * w0 + v1 * w1, a corner past the
        last plane not added)."""
        s = self.s
        tab = s['act_shift'].reshape(-1)
        D = tab.numel()
        lo, hi = s['xyz_min'], s['xyz_max']
        uz = ((pts[:, 2] - lo[2]) / (hi[2] - lo[2])) * 2 - 1
        iz = ((uz + 1) / 2) * (D - 1)
        f0 = torch.floor(iz)
        i0 = f0.long().clamp(0, D - 1)
        v = tab[i0] * ((f0 + 1) - iz)
        hi_ok = i0 + 1 <= D - 1
        v1 = tab[(i0 + 1).clamp(max=D - 1)] * (iz - f0)
        return torch.where(hi_ok, v + v1, v)

    # -- fused inference path ----------------------------------------------------------------------------------
    def fused_supported(self):
        """the fused march (ugrid_render_march_mpi) + shade kernels cover what BoundedRenderer.fused_supported lists -- (0, 9, 0)
        is configs/llff's net -- with mpi_depth <= 256 (the march stages act_shift in LDS)"""
        s = self.s
        return (super().fused_supported() and 2 <= int(s['mpi_depth']) <= 256
                and int(s['density_grid'].shape[4]) == int(s['mpi_depth']))

    frames_in_flight = 2      # run_render.render_viewpoints: views in flight on their own streams / work lists

    def _fused_state(self):
        st = self._bounded_state('mpi', {'act_shift': self.s['act_shift'].reshape(-1)})
        st['act_shift'] = 0.0          # the per-plane shift is part of the density; Raw2Alpha gets 0 (dmpigo.py:222,275)
        return st

    @torch.no_grad()
    def forward(self, rays_o, rays_d, viewdirs, global_step=None, **render_kwargs):
        s = self.s
        assert rays_o.dim() == 2 and rays_o.shape[-1] == 3, 'Only suuport point queries in [N, 3] format'
        assert render_kwargs.get('near', 0) == 0 and render_kwargs.get('far', 1) == 1
        N = rays_o.shape[0]
        dev = rays_o.device
        stepsize = render_kwargs['stepsize']
        n_samples = self.n_samples(stepsize)
        ray_pts, mask_outbbox = self.ru.sample_ndc_pts_on_rays(rays_o.contiguous(), rays_d.contiguous(), s['xyz_min'], s['xyz_max'],
                                                              n_samples)[:2]
        inb = ~mask_outbbox
        ray_pts = ray_pts[inb]
        ray_id = torch.arange(N, device=dev).view(-1, 1).expand_as(inb)[inb]
        step_id = torch.arange(n_samples, device=dev).view(1, -1).expand_as(inb)[inb]
        interval = stepsize * s['voxel_size_ratio']
        m = self.ru.maskcache_lookup(s['mask'], ray_pts.contiguous(), s['xyz2ijk_scale'], s['xyz2ijk_shift'])
        ray_pts, ray_id, step_id = ray_pts[m], ray_id[m], step_id[m]
        density = self.query(s['density_grid'], ray_pts, s['xyz_min'], s['xyz_max'], 0) + self.act_shift_at(ray_pts)
        alpha = self.ru.raw2alpha(density.flatten().contiguous(), 0, interval)[1]
        thres = float(s['fast_color_thres'])
        if thres > 0:
            k = alpha > thres
            ray_pts, ray_id, step_id, alpha = ray_pts[k], ray_id[k], step_id[k], alpha[k]
        weights, _, alphainv_last = self.ru.alpha2weight(alpha.contiguous(), ray_id.contiguous(), N)[:3]
        if thres > 0:
            k = weights > thres
            weights, alpha, ray_pts, ray_id, step_id = weights[k], alpha[k], ray_pts[k], ray_id[k], step_id[k]
        rgb, rgb_marched = self._colour(ray_pts, ray_id, weights, alphainv_last, viewdirs, N, render_kwargs['bg'])
        sv = (step_id + 0.5) / n_samples
        out = {'alphainv_last': alphainv_last, 'weights': weights, 'rgb_marched': rgb_marched, 'raw_alpha': alpha,
               'raw_rgb': rgb, 'ray_id': ray_id, 'n_max': n_samples, 's': sv}
        if render_kwargs.get('render_depth', False):
            out['depth'] = torch.zeros(N, device=dev).index_add_(0, ray_id, weights * sv)
        return out

    __call__ = forward
