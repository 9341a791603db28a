"""BoundedRenderer: what the renderers of the reference's three dense-grid models share -- DirectVoxGORenderer (dvgo_render),
DirectContractedVoxGORenderer (dcvgo_render), DirectMPIGORenderer (mpi_render).  Each of them has two paths with the same
outputs: `forward`, the reference's forward composed from the drop-in kernels (its sampling half is the subclass's own, its
colour half is `_colour` here), and `render_rays` / `render_view`, the fused march + shade kernels through a
FourierGridRenderer built on first use from the subclass's `_fused_state()` (`_bounded_state` + what differs).

A subclass sets `output_keys` (what render_rays returns), `ndc` / `ray_order` (how render_view makes and orders its rays),
`frames_in_flight`, and overrides `rgbnet_residual` and `fused_supported` where its model has a rule of its own.
"""
import torch
import torch.nn.functional as F


def bake_tensorf_checkpoint(ckpt, device, mem_get_info=None):
    """A checkpoint of a model with TensoRF grids (grid.TensoRFGrid: `density.xy_plane` ... `k0.f_vec`) as the checkpoint of the
    same model with dense grids: every TensoRF grid is baked ON `device` by one kernel (grid.tensorf_bake -- exact: trilinear weights
    are separable, so trilinear interpolation of the baked grid equals the factorised interpolation term by term) into the canonical
    [1,C,X,Y,Z] layout the brick packer reads; a dense grid passes through.  The renderers' existing state functions, fused march and
    shade kernels then apply unchanged.
    Before baking, the baked byte count is compared with the device's free memory (mem_get_info(device) -> (free, total), default
    torch.cuda.mem_get_info): RuntimeError naming both numbers if it does not fit."""
    from . import grid as _grid
    kw, sd = dict(ckpt['model_kwargs']), dict(ckpt['model_state_dict'])
    dev = torch.device(device)
    todo = [g for g in ('density', 'k0') if kw.get(g + '_type', 'DenseGrid') == 'TensoRFGrid']
    if not todo:
        raise ValueError("no TensoRFGrid in this checkpoint: use from_reference_checkpoint")
    shapes = {}
    for g in todo:
        X, Y = sd[g + '.xy_plane'].shape[2:]
        Z = sd[g + '.xz_plane'].shape[3]
        C = sd[g + '.f_vec'].shape[1] if g + '.f_vec' in sd else 1
        shapes[g] = (int(C), int(X), int(Y), int(Z))
    need = sum(4 * c * x * y * z for c, x, y, z in shapes.values())
    free = int((mem_get_info or torch.cuda.mem_get_info)(dev)[0])
    if need > free:
        raise RuntimeError("baking the TensoRF grids %s of this checkpoint needs %d bytes on %s, %d bytes are free" % (
            ", ".join("%s %s" % (g, list(shapes[g])) for g in todo), need, dev, free))
    for g in todo:
        factors = tuple(sd.pop(g + '.' + n).to(dev, torch.float32).contiguous() for n in _grid.TENSORF_FACTORS)
        f_vec = sd.pop(g + '.f_vec').to(dev, torch.float32).contiguous() if g + '.f_vec' in sd else None
        sd[g + '.grid'] = _grid.tensorf_bake(factors, f_vec)
        kw[g + '_type'], kw[g + '_config'] = 'DenseGrid', {}
    return {'model_kwargs': kw, 'model_state_dict': sd}


def stored_buffers_win(state, ckpt, keys):
    """`state` with the model's stored buffers in place of the values re-derived from `model_kwargs`.  The trainer changes them after
    construction, and the reference reloads them with the state dict (utils.load_model): `act_shift` is lowered by decay_after_scale at
    every pg_scale step (run_train.py:201), and DirectContractedVoxGO.get_kwargs saves the CONTRACTED bounds as xyz_min / xyz_max
    (dcvgo.py:139-141), from which scene_center / scene_radius cannot be re-derived.  A state built without them renders another
    scene than the one trained (colours off by up to 0.28 on the checkpoints of tests/test_gpu_tensorf_model.py)."""
    sd = ckpt['model_state_dict']
    for k in keys:
        if k in sd:
            state[k] = sd[k].detach().clone().float()
    return state


class BoundedRenderer:
    output_keys = ('rgb_marched', 'depth', 'alphainv_last')     # per-ray outputs the render program consumes (run_render.py:46)
    ndc = False               # render_view: forward-facing NDC rays
    ray_order = None          # render_view: FourierGridRenderer's ray_order for the fused path (None: its default, "auto")
    rgbnet_residual = False   # rgbnet on [k0[3:], embedding], k0[:3] added to its output (DirectVoxGO without rgbnet_direct)

    def __init__(self, state, device, ops=None, query=None, grad_query=None, mlp_mode=None):
        dev = torch.device(device)
        if ops is None:
            if dev.type != "cuda":
                raise RuntimeError("%s needs a HIP device (no CPU path)" % type(self).__name__)
            from . import render_utils_cuda, ub360_utils_cuda       # (importing them loads libugrid_hip.so)
            from .grid import GridQuery, grid_query
            self.ru, self.ub, self.query, self.grad_query = render_utils_cuda, ub360_utils_cuda, grid_query, GridQuery.apply
        else:                                   # tests: another implementation of the extension modules
            self.ru, self.ub = ops.render_utils_cuda, getattr(ops, 'ub360_utils_cuda', None)
            self.query, self.grad_query = query, grad_query or query
        self.device = dev
        self.s = {k: (v.to(dev).contiguous() if torch.is_tensor(v) else
                      ([x.to(dev).contiguous() for x in v] if isinstance(v, list) else v)) for k, v in state.items()}
        self.viewfreq = torch.tensor([float(2 ** i) for i in range(int(state["viewbase_pe"]))], device=dev)
        self.mlp_mode = mlp_mode
        self._fused = None if ops is None else False      # fused render kernels: HIP library only, built on first use

    # -- fused inference path ----------------------------------------------------------------------------------
    def fused_supported(self):
        """the fused march + shade kernels cover: the default HIP ops, fast_color_thres > 0, one resolution for both grids, and
        either no rgbnet (3-channel k0, rgb = sigmoid(k0)) or a depth-3 rgbnet (width <= 128) on [k0, view embedding] whose
        (0, C, viewbase_pe) ugrid_shade_supported lists"""
        if self._fused is False:
            return False
        s = self.s
        if float(s['fast_color_thres']) <= 0 or tuple(s['density_grid'].shape[2:]) != tuple(s['k0_grid'].shape[2:]):
            return False
        C = int(s['k0_grid'].shape[1])
        if len(s['rgbnet_weights']) == 0:
            return C == 3
        from . import _lib
        from .fourier_render import rgbnet_fits_fused
        w = s['rgbnet_weights']
        c_in = C - 3 if self.rgbnet_residual else C
        return (rgbnet_fits_fused(w) and w[0].shape[1] == c_in + 3 + 6 * int(s['viewbase_pe'])
                and bool(_lib.load().ugrid_shade_supported(0, C, int(s['viewbase_pe']))))

    def _bounded_state(self, variant, extra=None):
        """FourierGridRenderer's `state` for this model: the grids and the rgbnet, single-level (fourier_freq_num = 0), and
        state[variant] = the mask cache + `extra`.  The scene keys are those of a BOUNDED model (the box itself, no contraction);
        a subclass replaces what differs."""
        s = self.s
        lo, hi = s['xyz_min'], s['xyz_max']
        return {'density_grid': s['density_grid'], 'k0_grid': s['k0_grid'], 'rgbnet_weights': s['rgbnet_weights'],
                'rgbnet_biases': s['rgbnet_biases'], 'scene_center': (lo + hi) * 0.5, 'scene_radius': (hi - lo) * 0.5,
                'xyz_min': lo, 'xyz_max': hi, 'bg_len': 0.0, 'fourier_freq_num': 0, 'viewbase_pe': s['viewbase_pe'],
                'voxel_size_ratio': float(s['voxel_size_ratio']), 'fast_color_thres': float(s['fast_color_thres']),
                'contracted_norm': 'inf', 'world_len': 0,
                variant: dict({'mask': s['mask'], 'xyz2ijk_scale': s['xyz2ijk_scale'], 'xyz2ijk_shift': s['xyz2ijk_shift']},
                              **(extra or {}))}

    def _fused_renderer(self):
        """the fused march + shade renderer over this model's grids (built on first use)"""
        if self._fused is None:
            from .fourier_render import FourierGridRenderer
            self._fused = FourierGridRenderer(self._fused_state(), self.device, mlp_mode=self.mlp_mode)
        return self._fused

    def use_workspace_slot(self, k):
        """Views in flight on several streams take a work list each (run_render.render_viewpoints, FourierGridRenderer.use_workspace_slot);
        False: this model renders through the composed forward, one stream."""
        if not self.fused_supported():
            return False
        self._fused_renderer().use_workspace_slot(k)
        return True

    @torch.no_grad()
    def render_rays(self, rays_o, rays_d, viewdirs, **render_kwargs):
        """Per-ray outputs of forward() -- `output_keys` -- through the FUSED kernels: the reference's whole forward in two
        launches, no boolean-mask compactions, no host syncs.  Falls back to forward() for models outside fused_supported().
        render_kwargs as forward(), plus FourierGridRenderer's ray_order."""
        if not self.fused_supported():
            out = self.forward(rays_o, rays_d, viewdirs, **render_kwargs)
        else:
            kw = dict(render_kwargs)
            if 'bg' in kw and torch.is_tensor(kw['bg']):
                kw['bg'] = kw['bg'].to(self.device)
            out = self._fused_renderer()(rays_o.contiguous(), rays_d.contiguous(), viewdirs.contiguous(), **kw)
        return {k: out[k] for k in self.output_keys if k in out}

    def render_view(self, H, W, K, c2w, inverse_y=False, flip_x=False, flip_y=False, **render_kwargs):
        """One whole view through render_rays (fourier_render.render_view_of: rays generated on the device in 8 x 8 pixel
        blocks): {key: [H,W(,3)]} of the per-ray outputs."""
        from .fourier_render import render_view_of
        if not self.fused_supported():      # the composed forward takes no ray_order
            rr = lambda o, d, v, ray_order=None, **kw: self.render_rays(o, d, v, **kw)
        elif self.ray_order is None:
            rr = self.render_rays
        else:
            rr = lambda o, d, v, ray_order=self.ray_order, **kw: self.render_rays(o, d, v, ray_order=ray_order, **kw)
        return render_view_of(rr, self.device, H, W, K, c2w, inverse_y=inverse_y, flip_x=flip_x, flip_y=flip_y, ndc=self.ndc,
                              **render_kwargs)

    # -- the colour half of the composed forward ---------------------------------------------------------------
    def _colour(self, ray_pts, ray_id, weights, alphainv_last, viewdirs, N, bg):
        """k0 query -> rgbnet on [k0, view embedding] (or sigmoid(k0)) -> rgb_marched = per-ray sum of w * rgb + alphainv_last * bg
        (dvgo.py:378-406, dcvgo.py:331-353, dmpigo.py:297-318); returns (rgb per sample, rgb_marched [N,3])"""
        s = self.s
        k0 = self.query(s['k0_grid'], ray_pts, s['xyz_min'], s['xyz_max'], 0)
        if k0.dim() == 1:
            k0 = k0.unsqueeze(-1)
        if len(s['rgbnet_weights']) == 0:
            rgb = torch.sigmoid(k0)
        else:
            e = (viewdirs.unsqueeze(-1) * self.viewfreq).flatten(-2)
            emb = torch.cat([viewdirs, e.sin(), e.cos()], -1)[ray_id]
            h = torch.cat([k0[:, 3:] if self.rgbnet_residual else k0, emb], -1)
            n = len(s['rgbnet_weights'])
            for i in range(n):
                h = F.linear(h, s['rgbnet_weights'][i], s['rgbnet_biases'][i])
                if i + 1 < n:
                    h = torch.relu(h)
            rgb = torch.sigmoid(h + k0[:, :3] if self.rgbnet_residual else h)
        rgb_marched = torch.zeros(N, 3, device=weights.device).index_add_(0, ray_id, weights.unsqueeze(-1) * rgb)
        rgb_marched += alphainv_last.unsqueeze(-1) * bg
        return rgb, rgb_marched
