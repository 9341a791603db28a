"""Voxel-grid queries on the canonical [P,C,X,Y,Z] layout:
  grid_query     <- FourierGrid.forward (FourierGrid_grid.py:60-78) / DenseGrid.forward (grid.py:50-61), no autograd
  GridQuery      the same lookup as an autograd.Function: HIP forward + HIP scatter backward into the grid
                 (replaces F.grid_sample and its atomics-bound backward in training)
  FourierGrid    drop-in for the reference's nn.Module of that name (FourierGrid_grid.py:43-103): same constructor,
                 parameter / buffer names (state_dict compatible) and methods
  MaskGrid       <- MaskGrid.forward (grid.py:230-239, FourierGrid_grid.py:159-168)
  TrainMarch / TrainSample / TrainSampleVox / TrainSampleTensoRF
                 the fused sampling of the training forwards as autograd ops.  The sample ops differ in their input checks
                 and their march entry point only (TrainSampleTensoRF, over a factorised density, also in the lookup's backward):
                 what follows the march (_sample_stages) and the sampling's backward are one piece of code, and every op --
                 native_step.VoxGOStep included -- takes its per-(ray, slot) scratch from scratch()"""
import torch
import torch.nn.functional as F

from . import _gradpool, _lib, render_utils_cuda

_L = _lib.load()


@torch.no_grad()
def grid_query(grid, xyz, xyz_min, xyz_max, freq_num):
    """grid [P,C,X,Y,Z]; xyz [...,3] world coords -> [...,C] (squeezed if C==1).  freq_num=F>0: P=1+2F Fourier
    levels, mean over levels; freq_num<=0: plain dense grid (P=1).  Zero padding outside the grid."""
    cl = _lib.require_cuda_grid(("grid", grid))
    _lib.require_cuda(("xyz_min", xyz_min), ("xyz_max", xyz_max))
    _lib.require_f32(("grid", grid), ("xyz", xyz), ("xyz_min", xyz_min), ("xyz_max", xyz_max))
    if grid.dim() != 5:
        raise RuntimeError("grid must be [P,C,X,Y,Z]")
    P, C, X, Y, Z = grid.shape
    lead = xyz.shape[:-1]
    pts = xyz.reshape(-1, 3).contiguous()
    _lib.require_cuda(("xyz", pts))
    if pts.device != grid.device or xyz_min.device != grid.device or xyz_max.device != grid.device:
        raise RuntimeError("grid, xyz, xyz_min and xyz_max must be on the same device")
    out = torch.empty(pts.shape[0], C, dtype=torch.float32, device=grid.device)
    fn = _L.ugrid_grid_query_cl if cl else _L.ugrid_grid_query
    with _lib.guard(grid.device):
        _lib.check(fn(_lib.ptr(grid), P, C, X, Y, Z, _lib.ptr(pts), _lib.ptr(xyz_min),
                                       _lib.ptr(xyz_max), max(int(freq_num), 0), pts.shape[0], _lib.ptr(out),
                                       _lib.stream_of(grid)), "grid_query")
    out = out.reshape(*lead, C)
    return out.squeeze(-1) if C == 1 else out


class GridQuery(torch.autograd.Function):
    """out[..., C] = mean over the Fourier levels of trilinear(grid[l], level coordinates of xyz).  Differentiable in
    the grid only (the reference never differentiates the sample positions: rays carry no gradient)."""

    @staticmethod
    def forward(ctx, grid, xyz, xyz_min, xyz_max, freq_num):
        _lib.wait_pending(grid)      # an optimizer update of this grid may still run on a side stream (step(overlap=...))
        out = grid_query(grid, xyz, xyz_min, xyz_max, freq_num)
        if grid.requires_grad:
            ctx.save_for_backward(xyz.reshape(-1, 3).contiguous(), xyz_min, xyz_max)
            ctx.shape = tuple(grid.shape)
            ctx.freq_num = max(int(freq_num), 0)
            ctx.channels_last = _lib.is_channels_last(grid)    # the gradient is produced in the grid's own layout
            ctx.pool_key, ctx.grid_stride = _gradpool.key_of(grid), tuple(grid.stride())
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        pts, xyz_min, xyz_max = ctx.saved_tensors
        P, C, X, Y, Z = ctx.shape
        g = grad_out.reshape(-1, C).to(torch.float32).contiguous()
        grad_grid = _gradpool.take(ctx.pool_key, ctx.shape, ctx.grid_stride, g.device)    # all zero, from the last step
        if grad_grid is None:
            grad_grid = _lib.empty_like_grid(ctx.shape, ctx.channels_last, g.device, zero=True)
        # channel-last: the scatter also marks the 256-byte lines it adds to (the optimizer's masked passes visit only those)
        touch = _gradpool.touch_for_backward(ctx.pool_key, grad_grid, _L) if ctx.channels_last else None
        with _lib.guard(g.device):
            if touch is not None:
                _lib.check(_L.ugrid_grid_query_backward_cl_touch(
                    _lib.ptr(g), P, C, X, Y, Z, _lib.ptr(pts), _lib.ptr(xyz_min), _lib.ptr(xyz_max), ctx.freq_num, pts.shape[0],
                    _lib.ptr(grad_grid), _lib.ptr(touch), _lib.stream_of(g)), "grid_query_backward (touch)")
            else:
                fn = _L.ugrid_grid_query_backward_cl if ctx.channels_last else _L.ugrid_grid_query_backward
                _lib.check(fn(_lib.ptr(g), P, C, X, Y, Z, _lib.ptr(pts), _lib.ptr(xyz_min),
                              _lib.ptr(xyz_max), ctx.freq_num, pts.shape[0],
                              _lib.ptr(grad_grid), _lib.stream_of(g)), "grid_query_backward")
        return grad_grid, None, None, None, None


_scratch = {}      # width -> ((device, n), arrays)


def scratch(dev, n, width=5):
    """The march kernels' per-(ray, slot) scratch, kept between steps: points [n,3], density [n], step [n] i32 and, for the
    sample ops (width 5: TrainSample, TrainSampleVox, native_step.VoxGOStep), weight [n] and transmittance [n].  Written by
    the march and read by the compaction of the SAME forward (no backward takes it), so the ops share it; one ray-batch shape
    at a time per width: 8 + 4 * width bytes per (ray, slot)."""
    if _scratch.get(width, (None,))[0] != (dev, n):
        _scratch.pop(width, None)          # the old shape's arrays go before the new ones come
        _scratch[width] = ((dev, n), (torch.empty(n, 3, device=dev), torch.empty(n, device=dev),
                                      torch.empty(n, dtype=torch.int32, device=dev))
                           + tuple(torch.empty(n, device=dev) for _ in range(width - 3)))
    return _scratch[width][1]


class TrainMarch(torch.autograd.Function):
    """Fused stage 1 of the training forward (FourierGrid_model.py:554-598): rays -> the samples whose alpha exceeds
    fast_color_thres, compacted ray-major, with their raw densities -- sample_ray, the density lookup of all R*S points,
    Raw2Alpha, the mask and its boolean-index gathers in two kernels (ugrid_train_march / ugrid_train_compact) and ONE
    host read (the survivor count).  Differentiable in the density grid only: the backward scatters the M1 incoming
    density gradients with ugrid_grid_query_backward (the composed path runs that scatter over all R*S points).

    forward(grid [P,1,X,Y,Z], rays_o [R,3], rays_d [R,3], t [S], scene_center, scene_radius, xyz_min, xyz_max, bg_len,
            norm_l2, act_shift, interval, thres, freq_num) -> pts [M1,3], density [M1], ray_id [M1] i64, step_id [M1] i64,
            t [M1]"""

    @staticmethod
    def forward(ctx, grid, rays_o, rays_d, t, scene_center, scene_radius, xyz_min, xyz_max, bg_len, norm_l2, act_shift,
                interval, thres, freq_num):
        import ctypes
        _lib.wait_pending(grid)      # an optimizer update of this grid may still run on a side stream (step(overlap=...))
        _lib.require_cuda(("grid", grid), ("rays_o", rays_o), ("rays_d", rays_d), ("t", t), ("xyz_min", xyz_min), ("xyz_max", xyz_max))
        _lib.require_f32(("grid", grid), ("rays_o", rays_o), ("rays_d", rays_d), ("t", t))
        if grid.dim() != 5 or grid.shape[1] != 1:
            raise RuntimeError("density grid must be [P,1,X,Y,Z]")
        P, _, X, Y, Z = grid.shape
        R, S = rays_o.shape[0], t.numel()
        dev = grid.device
        sc = scratch(dev, R * S, width=3)
        count = torch.empty(R, dtype=torch.int32, device=dev)
        c3 = (ctypes.c_float * 3)(*[float(x) for x in scene_center])
        r3 = (ctypes.c_float * 3)(*[float(x) for x in scene_radius])
        F_ = max(int(freq_num), 0)
        with _lib.guard(dev):
            st = _lib.stream_of(grid)
            _lib.check(_L.ugrid_train_march(_lib.ptr(grid), P, X, Y, Z, F_, _lib.ptr(rays_o), _lib.ptr(rays_d), R, _lib.ptr(t), S,
                                            ctypes.cast(c3, ctypes.c_void_p), ctypes.cast(r3, ctypes.c_void_p), _lib.ptr(xyz_min),
                                            _lib.ptr(xyz_max), float(bg_len), int(bool(norm_l2)), float(act_shift), float(interval),
                                            float(thres), _lib.ptr(sc[0]), _lib.ptr(sc[1]), _lib.ptr(sc[2]), _lib.ptr(count), st),
                       "train_march")
            off = torch.cumsum(count, 0, dtype=torch.int64)
            M1 = int(off[-1].item()) if R > 0 else 0
            pts = torch.empty(M1, 3, device=dev)
            dens = torch.empty(M1, device=dev)
            ray_id = torch.empty(M1, dtype=torch.int64, device=dev)
            step_id = torch.empty(M1, dtype=torch.int64, device=dev)
            tt = torch.empty(M1, device=dev)
            if M1 > 0:
                _lib.check(_L.ugrid_train_compact(R, S, _lib.ptr(sc[0]), _lib.ptr(sc[1]), _lib.ptr(sc[2]), _lib.ptr(count),
                                                  _lib.ptr(off), _lib.ptr(t), _lib.ptr(pts), _lib.ptr(dens), _lib.ptr(ray_id),
                                                  _lib.ptr(step_id), _lib.ptr(tt), st), "train_compact")
        ctx.save_for_backward(pts, xyz_min, xyz_max)
        ctx.shape, ctx.freq_num = tuple(grid.shape), F_
        ctx.pool_key, ctx.grid_stride = _gradpool.key_of(grid), tuple(grid.stride())
        ctx.mark_non_differentiable(pts, ray_id, step_id, tt)
        return pts, dens, ray_id, step_id, tt

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pts, g_dens, g_ray, g_step, g_t):
        pts, xyz_min, xyz_max = ctx.saved_tensors
        P, C, X, Y, Z = ctx.shape
        grad_grid = _gradpool.take(ctx.pool_key, ctx.shape, ctx.grid_stride, pts.device)
        if grad_grid is None:
            grad_grid = torch.zeros(ctx.shape, dtype=torch.float32, device=pts.device)
        if pts.shape[0] > 0:
            g = g_dens.reshape(-1, 1).to(torch.float32).contiguous()
            with _lib.guard(g.device):
                _lib.check(_L.ugrid_grid_query_backward(_lib.ptr(g), P, C, X, Y, Z, _lib.ptr(pts), _lib.ptr(xyz_min), _lib.ptr(xyz_max),
                                                        ctx.freq_num, pts.shape[0], _lib.ptr(grad_grid), _lib.stream_of(g)),
                           "grid_query_backward")
        return (grad_grid,) + (None,) * 13


class TrainSample(torch.autograd.Function):
    """Stages 1 and 2 of the training forward's sampling (FourierGrid_model.py:554-629) as ONE op: TrainMarch, Raw2Alpha,
    Alphas2Weights, the weight mask and its gathers -- include/ugrid_hip.h: ugrid_train_sample / _compact / _backward.  One
    march kernel (a ray ends where its transmittance does), one cumsum + ONE host read (M1, M2), one compaction
    (_sample_stages); the backward is one pass over the stage-1 samples + the density lookup's scatter.  Returns the stage-2
    samples (pts, raw density, alpha, weights, ray_id, step_id, t) and alphainv_last [R]; differentiable in the density grid
    through `weights`, `alphainv_last` and the raw `density` output."""

    @staticmethod
    def forward(ctx, grid, rays_o, rays_d, t, scene_center, scene_radius, xyz_min, xyz_max, bg_len, norm_l2, act_shift,
                interval, thres, freq_num):
        import ctypes
        _lib.wait_pending(grid)
        _lib.require_cuda(("grid", grid), ("rays_o", rays_o), ("rays_d", rays_d), ("t", t), ("xyz_min", xyz_min), ("xyz_max", xyz_max))
        _lib.require_f32(("grid", grid), ("rays_o", rays_o), ("rays_d", rays_d), ("t", t))
        if grid.dim() != 5 or grid.shape[1] != 1:
            raise RuntimeError("density grid must be [P,1,X,Y,Z]")
        P, _, X, Y, Z = grid.shape
        R, S = rays_o.shape[0], t.numel()
        c3 = (ctypes.c_float * 3)(*[float(x) for x in scene_center])
        r3 = (ctypes.c_float * 3)(*[float(x) for x in scene_radius])
        F_ = max(int(freq_num), 0)
        consts = (float(act_shift), float(interval), float(thres))

        def march(*outs):
            _lib.check(_L.ugrid_train_sample(_lib.ptr(grid), P, X, Y, Z, F_, _lib.ptr(rays_o), _lib.ptr(rays_d), R, _lib.ptr(t), S,
                                             ctypes.cast(c3, ctypes.c_void_p), ctypes.cast(r3, ctypes.c_void_p), _lib.ptr(xyz_min),
                                             _lib.ptr(xyz_max), float(bg_len), int(bool(norm_l2)), *consts, *outs), "train_sample")
        return _sample_stages(ctx, grid, R, S, t, xyz_min, xyz_max, consts, F_, march, vox=False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pts, g_dens2, g_alpha, g_w2, g_ainv, *g_rest):
        pts1, dens1, w1, T1, pos2, counts, off, ainv, xyz_min, xyz_max = ctx.saved_tensors
        P, C, X, Y, Z = ctx.shape
        dev = pts1.device
        grad_grid = _gradpool.take(ctx.pool_key, ctx.shape, ctx.grid_stride, dev)
        if grad_grid is None:
            grad_grid = torch.zeros(ctx.shape, dtype=torch.float32, device=dev)
        M1, R = pts1.shape[0], ainv.shape[0]
        if M1 > 0:
            f32 = lambda g: None if g is None else g.to(torch.float32).contiguous()
            g_dens2, g_w2, g_ainv = f32(g_dens2), f32(g_w2), f32(g_ainv)
            g1 = torch.empty(M1, 1, device=dev)
            with _lib.guard(dev):
                st = _lib.stream_of(pts1)
                _lib.check(_L.ugrid_train_sample_backward(R, ctx.consts[0], ctx.consts[1], _lib.ptr(dens1), _lib.ptr(w1), _lib.ptr(T1),
                                                          _lib.ptr(pos2), _lib.ptr(counts[0]), _lib.ptr(off[0]), _lib.ptr(ainv),
                                                          _lib.ptr(g_w2), _lib.ptr(g_ainv), _lib.ptr(g_dens2), _lib.ptr(g1), st),
                           "train_sample_backward")
                _lib.check(_L.ugrid_grid_query_backward(_lib.ptr(g1), P, C, X, Y, Z, _lib.ptr(pts1), _lib.ptr(xyz_min), _lib.ptr(xyz_max),
                                                        ctx.freq_num, M1, _lib.ptr(grad_grid), st), "grid_query_backward")
        return (grad_grid,) + (None,) * (len(ctx.needs_input_grad) - 1)      # (this forward's inputs or TrainSampleVox's)


class TrainSampleVox(TrainSample):
    """TrainSample for the reference's dense-grid models: the sampling of DirectContractedVoxGO.forward (dcvgo.py:228-330,
    cfg['mode'] == 'dcvgo'), of DirectVoxGO.forward (dvgo.py:306-375, 'dvgo') and of DirectMPIGO.forward (dmpigo.py:224-292, 'mpi')
    as one march + one compaction (include/ugrid_hip.h: ugrid_train_sample_dcvgo / _dvgo / _mpi / _compact_vox), differentiable in the density grid through
    `weights`, `alphainv_last` and the raw `density` output -- the backward is TrainSample's, inherited (ugrid_train_sample_backward
    + the lookup's scatter).

    forward(grid [1,1,X,Y,Z], rays_o [R,3], rays_d [R,3], t [S] or None, xyz_min, xyz_max, mask [mi,mj,mk] bool, cfg) ->
        pts [M2,3], density [M2], alpha [M2], weights [M2], alphainv_last [R], ray_id [M2] i64, step_id [M2] i64, t [M2]
        (dvgo, mpi: float(step_id)), inner [M2] bool (dvgo, mpi: all True)
    cfg (host values): mode, act_shift, interval, thres, mask_scale[3], mask_shift[3] and
        dcvgo: scene_center[3], scene_radius[3], bg_len, norm_l2, dist_thres;   dvgo: near, far, stepdist, slots;
        mpi: n_steps, mpi_depth and act_shift = the DEVICE tensor of the per-plane shift ([mpi_depth] values: it is part of the
             density the march stores -- the returned `density` is grid + shift -- and Raw2Alpha's own shift is 0)"""

    @staticmethod
    def forward(ctx, grid, rays_o, rays_d, t, xyz_min, xyz_max, mask, cfg):
        _lib.wait_pending(grid)
        _lib.require_cuda(("grid", grid))
        _lib.require_f32(("grid", grid))
        if grid.dim() != 5 or grid.shape[0] != 1 or grid.shape[1] != 1 or not grid.is_contiguous():
            raise RuntimeError("density grid must be a contiguous [1,1,X,Y,Z]")
        R, S, consts, march = _vox_march((_lib.ptr(grid), *grid.shape[2:]), "", grid.device, rays_o, rays_d, t, xyz_min, xyz_max, mask, cfg)
        return _sample_stages(ctx, grid, R, S, t if cfg['mode'] == 'dcvgo' else None, xyz_min, xyz_max, consts, 0, march, vox=True)


def _vox_march(density_args, suffix, dev, rays_o, rays_d, t, xyz_min, xyz_max, mask, cfg):
    """What TrainSampleVox and TrainSampleTensoRF share behind the checks of their density: the checks of the rays, the mask and the
    mode's own inputs, and the march entry point ugrid_train_sample_<mode><suffix> bound to everything but its outputs.
    density_args: what that entry point takes for the density (grid pointer, X, Y, Z; suffix "_tensorf": the six factor pointers, X,
    Y, Z, R, Rxy, comp_last -- 'dvgo' and 'dcvgo' only); dev: the density's device.  -> R, S (scratch slots per ray), consts (shift,
    interval, thres), march(*pointers of the scratch, the counts and alphainv_last, stream)"""
    import ctypes
    _lib.require_cuda(("rays_o", rays_o), ("rays_d", rays_d), ("xyz_min", xyz_min), ("xyz_max", xyz_max), ("mask", mask))
    _lib.require_f32(("rays_o", rays_o), ("rays_d", rays_d))
    if mask.dtype != torch.bool or mask.dim() != 3 or not mask.is_contiguous():
        raise RuntimeError("mask must be a contiguous bool [mi,mj,mk]")
    mode = cfg['mode']
    R = rays_o.shape[0]
    if mode == 'dcvgo':
        _lib.require_cuda(("t", t))
        _lib.require_f32(("t", t))
        S = t.numel()
    elif mode == 'dvgo':
        S = int(cfg['slots'])
    elif mode == 'mpi' and not suffix:
        S, D = int(cfg['n_steps']), int(cfg['mpi_depth'])
        tab = cfg['act_shift']
        _lib.require_cuda(("act_shift", tab))
        _lib.require_f32(("act_shift", tab))
        if S < 2 or not 1 <= D <= 256 or tab.numel() != D or not tab.is_contiguous() or tab.device != dev:
            raise RuntimeError("mpi: n_steps >= 2, 1 <= mpi_depth <= 256 and a contiguous act_shift of mpi_depth values on the grid's device")
    else:
        raise ValueError(mode)
    f3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])
    md = (ctypes.c_int32 * 3)(*[int(x) for x in mask.shape])
    ms, mh = f3(cfg['mask_scale']), f3(cfg['mask_shift'])
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    consts = (0.0 if mode == 'mpi' else float(cfg['act_shift']), float(cfg['interval']), float(cfg['thres']))
    rays = (_lib.ptr(rays_o), _lib.ptr(rays_d), R)
    mask_args = (_lib.ptr(mask), vp(md), vp(ms), vp(mh))
    host = [md, ms, mh]          # (the host arrays behind the pointers live as long as `march`)
    if mode == 'dcvgo':
        c3, r3 = f3(cfg['scene_center']), f3(cfg['scene_radius'])
        host += [c3, r3]
        args = (*rays, _lib.ptr(t), S, vp(c3), vp(r3), _lib.ptr(xyz_min), _lib.ptr(xyz_max), float(cfg['bg_len']), int(bool(cfg['norm_l2'])),
                float(cfg['dist_thres']), *mask_args, *consts)
    elif mode == 'mpi':
        args = (*rays, S, _lib.ptr(xyz_min), _lib.ptr(xyz_max), _lib.ptr(tab), D, *mask_args, consts[1], consts[2])
    else:
        args = (*rays, S, _lib.ptr(xyz_min), _lib.ptr(xyz_max), float(cfg['near']), float(cfg['far']), float(cfg['stepdist']), *mask_args, *consts)
    fn, what = getattr(_L, "ugrid_train_sample_%s%s" % (mode, suffix)), "train_sample_%s%s" % (mode, suffix)

    def march(*outs, _host=host):
        _lib.check(fn(*density_args, *args, *outs), what)
    return R, S, consts, march


def _sample_stages(ctx, grid, R, S, t, xyz_min, xyz_max, consts, freq_num, march, vox):
    """What TrainSample, TrainSampleVox and TrainSampleTensoRF do after their input checks: the scratch, `march(*pointers of the
    scratch, the two per-ray counts and alphainv_last, stream)` -- the caller's march entry point --, the cumsum and the ONE host
    read (M1, M2), the stage-1 / stage-2 arrays, the compaction (`vox`: ugrid_train_sample_compact_vox, which also writes the inner
    flags of the samples when there is a sample table `t`), and what the backwards read from ctx: the stage-1 arrays and
    ctx.consts always; of the density parameter -- `grid`: the 5-D grid, or the six factors of a TensoRF density -- the dense
    backward's shape, strides and gradient-pool key for a grid, nothing for factors (their op saves them itself)."""
    dense = torch.is_tensor(grid)
    dev = grid.device if dense else grid[0].device
    sc = scratch(dev, R * S)
    counts = torch.empty(2, R, dtype=torch.int32, device=dev)
    ainv = torch.empty(R, device=dev)
    shift, interval, thres = consts
    with _lib.guard(dev):
        st = _lib.stream_of(ainv)
        march(*[_lib.ptr(x) for x in sc], _lib.ptr(counts[0]), _lib.ptr(counts[1]), _lib.ptr(ainv), st)
        off = torch.cumsum(counts, 1, dtype=torch.int64)            # [2,R] inclusive
        M1, M2 = (int(x) for x in off[:, -1].tolist()) if R > 0 else (0, 0)     # the one host read
        pts1, dens1, w1, T1 = torch.empty(M1, 3, device=dev), torch.empty(M1, device=dev), torch.empty(M1, device=dev), \
            torch.empty(M1, device=dev)
        pos2 = torch.empty(M1, dtype=torch.int32, device=dev)
        pts2, dens2, alpha2, w2, tt2 = torch.empty(M2, 3, device=dev), torch.empty(M2, device=dev), torch.empty(M2, device=dev), \
            torch.empty(M2, device=dev), torch.empty(M2, device=dev)
        ray2, step2 = torch.empty(M2, dtype=torch.int64, device=dev), torch.empty(M2, dtype=torch.int64, device=dev)
        inner2 = (torch.ones(M2, dtype=torch.bool, device=dev),) if vox else ()
        if M1 > 0:
            tp = _lib.ptr(t) if t is not None else None
            args = (R, S, shift, interval, thres, *[_lib.ptr(x) for x in sc], _lib.ptr(counts[0]), _lib.ptr(off[0]), _lib.ptr(counts[1]),
                    _lib.ptr(off[1]), tp, _lib.ptr(pts1), _lib.ptr(dens1), _lib.ptr(w1), _lib.ptr(T1), _lib.ptr(pos2), _lib.ptr(pts2),
                    _lib.ptr(dens2), _lib.ptr(alpha2), _lib.ptr(w2), _lib.ptr(ray2), _lib.ptr(step2), _lib.ptr(tt2))
            if vox:
                _lib.check(_L.ugrid_train_sample_compact_vox(*args, _lib.ptr(inner2[0]) if t is not None else None, st),
                           "train_sample_compact_vox")
            else:
                _lib.check(_L.ugrid_train_sample_compact(*args, st), "train_sample_compact")
    ctx.save_for_backward(pts1, dens1, w1, T1, pos2, counts, off, ainv, xyz_min, xyz_max, *(() if dense else grid))
    ctx.freq_num, ctx.consts = freq_num, (shift, interval)
    if dense:
        ctx.shape = tuple(grid.shape)
        ctx.pool_key, ctx.grid_stride = _gradpool.key_of(grid), tuple(grid.stride())
    ctx.mark_non_differentiable(pts2, alpha2, ray2, step2, tt2, *inner2)
    return (pts2, dens2, alpha2, w2, ainv, ray2, step2, tt2) + inner2


def create_grid(type, **kwargs):
    """grid.py:30-36 of the reference: 'DenseGrid' (here FourierGrid without Fourier levels) or 'TensoRFGrid'"""
    if type == 'DenseGrid':
        kwargs.setdefault('use_nerf_pos', False)
        kwargs.setdefault('fourier_freq_num', 0)
        return FourierGrid(**kwargs)
    if type == 'TensoRFGrid':
        return TensoRFGrid(**kwargs)
    raise NotImplementedError


# ---------------------------------------------------------------------------------------------------------------------------
# TensoRF (vector-matrix) grids: grid.py:90-201 of the reference on csrc/ugrid_tensorf.hip
# ---------------------------------------------------------------------------------------------------------------------------
TENSORF_FACTORS = ('xy_plane', 'xz_plane', 'yz_plane', 'x_vec', 'y_vec', 'z_vec')


def _tensorf_args(factors, f_vec, world_size=None):
    """checks + (pointers of the six factors and f_vec), (X, Y, Z, R, Rxy, C), comp_last of one grid's tensors"""
    xy, xz, yz, xv, yv, zv = factors
    named = list(zip(TENSORF_FACTORS, factors)) + ([("f_vec", f_vec)] if f_vec is not None else [])
    _lib.require_f32(*named)
    if any(t.dim() != 4 or t.shape[0] != 1 for t in factors):
        raise RuntimeError("TensoRF factors are [1,R,A,B] planes and [1,R,N,1] vectors")
    Rxy, X, Y = xy.shape[1:]
    R, Z = xz.shape[1], xz.shape[3]
    want = {'xy_plane': (1, Rxy, X, Y), 'xz_plane': (1, R, X, Z), 'yz_plane': (1, R, Y, Z), 'x_vec': (1, R, X, 1), 'y_vec': (1, R, Y, 1),
            'z_vec': (1, Rxy, Z, 1)}
    for name, t in zip(TENSORF_FACTORS, factors):
        if tuple(t.shape) != want[name]:
            raise RuntimeError("%s is %s, expected %s" % (name, tuple(t.shape), want[name]))
    comp_last = any(_lib.is_comp_last(t) for t in factors)
    for name, t in zip(TENSORF_FACTORS, factors):
        if not (t.is_contiguous(memory_format=torch.channels_last) if comp_last else t.is_contiguous()):
            raise RuntimeError("%s must be contiguous (the six factors share one layout, canonical or component-last)" % name)
    for name, t in named:          # (after the shape and layout checks, which need no device)
        if not t.is_cuda or t.device != xy.device:
            raise RuntimeError("%s must be a CUDA tensor on the device of xy_plane" % name)
    C = 1
    if f_vec is not None:
        if f_vec.dim() != 2 or f_vec.shape[0] != R + R + Rxy or not f_vec.is_contiguous():
            raise RuntimeError("f_vec must be a contiguous [R+R+Rxy, C]")
        C = f_vec.shape[1]
    if not 1 <= C <= 16 or (2 * R + Rxy) * C > 3072:
        raise RuntimeError("TensoRF kernels: 1 <= channels <= 16 and (2 n_comp + n_comp_xy) * channels <= 3072 (got C=%d, R=%d, Rxy=%d)" % (C, R, Rxy))
    return [_lib.ptr(t) for t in factors] + [_lib.ptr(f_vec)], (X, Y, Z, R, Rxy, C), int(comp_last)


def _tensorf_points(xyz, xyz_min, xyz_max, dev):
    pts = xyz.reshape(-1, 3).contiguous()
    _lib.require_cuda(("xyz", pts), ("xyz_min", xyz_min), ("xyz_max", xyz_max))
    _lib.require_f32(("xyz", pts), ("xyz_min", xyz_min), ("xyz_max", xyz_max))
    if pts.device != dev or xyz_min.device != dev or xyz_max.device != dev:
        raise RuntimeError("the factors, xyz, xyz_min and xyz_max must be on the same device")
    return pts


@torch.no_grad()
def tensorf_query(factors, f_vec, xyz, xyz_min, xyz_max):
    """factors (xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec), f_vec [R+R+Rxy, C] or None (C == 1); xyz [..., 3] world
    coordinates -> [...] (C == 1) or [..., C]: TensoRFGrid.forward (grid.py:111-129), no autograd"""
    ptrs, dims, cl = _tensorf_args(factors, f_vec)
    C = dims[5]
    dev = factors[0].device
    pts = _tensorf_points(xyz, xyz_min, xyz_max, dev)
    out = torch.empty((pts.shape[0], C) if f_vec is not None else (pts.shape[0],), dtype=torch.float32, device=dev)
    with _lib.guard(dev):
        _lib.check(_L.ugrid_tensorf_query(*ptrs, *dims, cl, _lib.ptr(pts), _lib.ptr(xyz_min), _lib.ptr(xyz_max), pts.shape[0], _lib.ptr(out),
                                          _lib.stream_of(pts)), "tensorf_query")
    return out.reshape(*xyz.shape[:-1], C) if f_vec is not None else out.reshape(xyz.shape[:-1])


@torch.no_grad()
def tensorf_query_backward(grad_out, factors, f_vec, pts, xyz_min, xyz_max, grads=None):
    """gradients of tensorf_query's output w.r.t. the six factors and f_vec (None for C == 1), each in its tensor's own layout.
    grads: seven caller-allocated tensors to write into (tests); default: new ones"""
    ptrs, dims, cl = _tensorf_args(factors, f_vec)
    dev = factors[0].device
    pts = _tensorf_points(pts, xyz_min, xyz_max, dev)
    if grad_out.numel() != pts.shape[0] * dims[5]:
        raise RuntimeError("grad_out must be [n] or [n, C] on the factors' device")
    g = grad_out.reshape(pts.shape[0], dims[5]).to(torch.float32).contiguous()
    if g.device != dev:
        raise RuntimeError("grad_out must be [n] or [n, C] on the factors' device")
    if grads is None:
        grads = [torch.empty_like(t, memory_format=torch.preserve_format) for t in factors] + [torch.empty_like(f_vec) if f_vec is not None else None]
    with _lib.guard(dev):
        _lib.check(_L.ugrid_tensorf_query_backward(_lib.ptr(g), *ptrs, *dims, cl, _lib.ptr(pts), _lib.ptr(xyz_min), _lib.ptr(xyz_max),
                                                   pts.shape[0], *[_lib.ptr(t) for t in grads], _lib.stream_of(pts)), "tensorf_query_backward")
    return grads


@torch.no_grad()
def tensorf_tv_add_grad(factors, grads, wx, wy, wz):
    """adds the gradient of TensoRFGrid.total_variation_add_grad's loss (grid.py:142-154) to the six `grads` in place"""
    ptrs, dims, cl = _tensorf_args(factors, None)
    for (name, t), g in zip(zip(TENSORF_FACTORS, factors), grads):
        if g.dtype != torch.float32 or g.device != t.device or g.shape != t.shape or g.stride() != t.stride():
            raise RuntimeError("the gradient of %s must have its tensor's device, shape and layout" % name)
    with _lib.guard(factors[0].device):
        _lib.check(_L.ugrid_tensorf_tv_add_grad(*ptrs[:6], *[_lib.ptr(g) for g in grads], *dims[:5], cl, float(wx), float(wy), float(wz),
                                                _lib.stream_of(factors[0])), "tensorf_tv_add_grad")


@torch.no_grad()
def tensorf_bake(factors, f_vec, channels_last=False, out=None):
    """the dense [1,C,X,Y,Z] grid of TensoRFGrid.get_dense_grid (grid.py:156-169) in one kernel, no intermediate; channels_last:
    stored [X][Y][Z][C] (torch.channels_last_3d of the same logical tensor, FourierGrid's training layout); out: a tensor of an
    earlier call with the same arguments, written again instead of a new one"""
    ptrs, dims, cl = _tensorf_args(factors, f_vec)
    X, Y, Z, _, _, C = dims
    if out is None:
        out = _lib.empty_like_grid((1, C, X, Y, Z), bool(channels_last) and C > 1, factors[0].device)
    elif tuple(out.shape) != (1, C, X, Y, Z) or out.dtype != torch.float32 or out.device != factors[0].device \
            or _lib.is_channels_last(out) != (bool(channels_last) and C > 1) or not (out.is_contiguous() or _lib.is_channels_last(out)):
        raise RuntimeError("out must be the float32 [1,C,X,Y,Z] tensor of this bake, in the layout asked for")
    with _lib.guard(out.device):
        _lib.check(_L.ugrid_tensorf_bake(*ptrs, *dims, cl, int(bool(channels_last) and C > 1), _lib.ptr(out), _lib.stream_of(out)), "tensorf_bake")
    return out


def tensorf_compose(factors, f_vec, xyz, xyz_min, xyz_max):
    """The same lookup as a torch composition (six grid_sample calls, a concatenation and a product with f_vec), differentiable by
    autograd on any device: the stand-in of the tests' CPU oracle (TensoRFGrid.query_fn) and the baseline of tools/bench_tensorf.py"""
    xy, xz, yz, xv, yv, zv = factors
    u = ((xyz.reshape(1, 1, -1, 3) - xyz_min) / (xyz_max - xyz_min)) * 2 - 1
    u = torch.cat([u, torch.zeros_like(u[..., :1])], -1)

    def tap(t, cols):
        return F.grid_sample(t, u[..., cols], mode='bilinear', align_corners=True).flatten(0, 2).T
    feats = [tap(xy, [1, 0]) * tap(zv, [3, 2]), tap(xz, [2, 0]) * tap(yv, [3, 1]), tap(yz, [2, 1]) * tap(xv, [3, 0])]
    if f_vec is None:
        return (feats[0].sum(-1) + feats[1].sum(-1) + feats[2].sum(-1)).reshape(xyz.shape[:-1])
    return torch.mm(torch.cat(feats, -1), f_vec).reshape(*xyz.shape[:-1], f_vec.shape[1])


class TrainSampleTensoRF(torch.autograd.Function):
    """TrainSampleVox for a TensoRF DENSITY (cfg['mode'] 'dvgo' or 'dcvgo'): the same march with the factorised lookup in place of
    the eight-corner gather (include/ugrid_hip.h: ugrid_train_sample_dvgo_tensorf / _dcvgo_tensorf; the density it returns is, bit
    for bit, tensorf_query's at the returned points), the same compaction, the same nine outputs.  The backward is
    ugrid_train_sample_backward over the M1 stage-1 samples, then the factorised lookup's backward (ugrid_tensorf_query_backward)
    over those M1 points only: six gradients, each in its factor's own layout (new tensors: TensoRF factors stay out of _gradpool).

    forward(xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, rays_o [R,3], rays_d [R,3], t [S] or None, xyz_min, xyz_max,
            mask [mi,mj,mk] bool, cfg) -- cfg as TrainSampleVox takes it for the mode."""

    @staticmethod
    def forward(ctx, xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, rays_o, rays_d, t, xyz_min, xyz_max, mask, cfg):
        factors = (xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec)
        for p in factors:
            _lib.wait_pending(p)
        ptrs, dims, cl = _tensorf_args(factors, None)
        R, S, consts, march = _vox_march((*ptrs[:6], *dims[:5], cl), "_tensorf", xy_plane.device, rays_o, rays_d, t, xyz_min, xyz_max, mask, cfg)
        if any(x.device != xy_plane.device for x in (rays_o, rays_d, xyz_min, xyz_max, mask)):
            raise RuntimeError("the factors, rays_o, rays_d, xyz_min, xyz_max and mask must be on the same device")
        return _sample_stages(ctx, factors, R, S, t if cfg['mode'] == 'dcvgo' else None, xyz_min, xyz_max, consts, 0, march, vox=True)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pts, g_dens2, g_alpha, g_w2, g_ainv, *g_rest):
        pts1, dens1, w1, T1, pos2, counts, off, ainv, xyz_min, xyz_max, *factors = ctx.saved_tensors
        dev = pts1.device
        M1, R = pts1.shape[0], ainv.shape[0]
        if M1 == 0:          # no sample took part in the forward: zero gradients, nothing launched
            grads = [torch.zeros_like(p, memory_format=torch.preserve_format) for p in factors]
        else:
            f32 = lambda g: None if g is None else g.to(torch.float32).contiguous()
            g_dens2, g_w2, g_ainv = f32(g_dens2), f32(g_w2), f32(g_ainv)
            g1 = torch.empty(M1, device=dev)
            with _lib.guard(dev):
                _lib.check(_L.ugrid_train_sample_backward(R, ctx.consts[0], ctx.consts[1], _lib.ptr(dens1), _lib.ptr(w1), _lib.ptr(T1),
                                                          _lib.ptr(pos2), _lib.ptr(counts[0]), _lib.ptr(off[0]), _lib.ptr(ainv),
                                                          _lib.ptr(g_w2), _lib.ptr(g_ainv), _lib.ptr(g_dens2), _lib.ptr(g1),
                                                          _lib.stream_of(pts1)), "train_sample_backward")
            grads = tensorf_query_backward(g1, factors, None, pts1, xyz_min, xyz_max)[:6]
        return tuple(grads) + (None,) * 7


class TensoRFQuery(torch.autograd.Function):
    """tensorf_query as an autograd op: HIP forward, HIP backward into the six factors and f_vec (the interpolants are recomputed; only
    the points are kept).  forward(xyz, xyz_min, xyz_max, xy_plane, xz_plane, yz_plane, x_vec, y_vec, z_vec, f_vec or None).
    xyz gets NO gradient (None): like every lookup of this package -- rays carry none in the reference's training."""

    @staticmethod
    def forward(ctx, xyz, xyz_min, xyz_max, *tensors):
        factors, f_vec = tensors[:6], tensors[6]
        out = tensorf_query(factors, f_vec, xyz, xyz_min, xyz_max)
        ctx.save_for_backward(xyz.reshape(-1, 3).contiguous(), xyz_min, xyz_max, *[t for t in tensors if t is not None])
        ctx.has_f = f_vec is not None
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        pts, xyz_min, xyz_max, *tensors = ctx.saved_tensors
        grads = tensorf_query_backward(grad_out, tensors[:6], tensors[6] if ctx.has_f else None, pts, xyz_min, xyz_max)
        return (None, None, None) + tuple(grads)


class TensoRFGrid(torch.nn.Module):
    """Vector-matrix decomposed grid; mirrors the reference's TensoRFGrid (grid.py:90-201): same constructor arguments, parameter
    names and logical shapes (state_dict compatible), initialisation and methods, with the lookup, its backward, the total-variation
    gradient and the dense bake on the HIP kernels.  `component_last = True` STORES the factors component-last (torch.channels_last
    of the same logical [1,R,A,B] tensors: a texel's R components are one run; state dicts and checkpoints are unchanged).  The
    default is the canonical layout: at configs/nerf/ship.tensorf.py's final shape the k0 query measured 0.16 ms canonical against
    0.52 ms component-last, the density query 0.48 against 0.43 (profiles/tensorf/query.json)."""

    component_last = False
    # test hooks, as FourierGrid's: query_fn(factors, f_vec, xyz, xyz_min, xyz_max) (differentiable; e.g. tensorf_compose) and
    # tv_module.tensorf_tv_add_grad(factors, grads, wx, wy, wz); None = the HIP kernels
    query_fn = None
    tv_module = None

    def __init__(self, channels, world_size, xyz_min, xyz_max, config, component_last=None):
        super().__init__()
        self.channels = channels
        self.world_size = world_size
        self.config = config
        if component_last is not None:
            self.component_last = bool(component_last)
        self.register_buffer('xyz_min', torch.Tensor(xyz_min))
        self.register_buffer('xyz_max', torch.Tensor(xyz_max))
        X, Y, Z = [int(v) for v in world_size]
        R = config['n_comp']
        Rxy = config.get('n_comp_xy', R)
        # (the reference's draws, in its order: the same generator state gives the same factors)
        self.xy_plane = torch.nn.Parameter(self._as_stored(torch.randn([1, Rxy, X, Y]) * 0.1))
        self.xz_plane = torch.nn.Parameter(self._as_stored(torch.randn([1, R, X, Z]) * 0.1))
        self.yz_plane = torch.nn.Parameter(self._as_stored(torch.randn([1, R, Y, Z]) * 0.1))
        self.x_vec = torch.nn.Parameter(self._as_stored(torch.randn([1, R, X, 1]) * 0.1))
        self.y_vec = torch.nn.Parameter(self._as_stored(torch.randn([1, R, Y, 1]) * 0.1))
        self.z_vec = torch.nn.Parameter(self._as_stored(torch.randn([1, Rxy, Z, 1]) * 0.1))
        if self.channels > 1:
            self.f_vec = torch.nn.Parameter(torch.ones([R + R + Rxy, channels]))
            torch.nn.init.kaiming_uniform_(self.f_vec, a=5 ** 0.5)

    def _as_stored(self, t):
        return t.contiguous(memory_format=torch.channels_last) if self.component_last else t.contiguous()

    def factors(self):
        return tuple(getattr(self, n) for n in TENSORF_FACTORS)

    def _f_vec(self):
        return self.f_vec if self.channels > 1 else None

    def forward(self, xyz):
        """xyz [..., 3] world coordinates -> [..., C] ([...] when C == 1)"""
        if self.query_fn is not None:
            return self.query_fn(self.factors(), self._f_vec(), xyz, self.xyz_min, self.xyz_max)
        return TensoRFQuery.apply(xyz, self.xyz_min, self.xyz_max, *self.factors(), self._f_vec())

    def scale_volume_grid(self, new_world_size):
        """six bilinear resamplings, as the reference (grid.py:131-140); once per pg_scale step"""
        if self.channels == 0:
            return
        X, Y, Z = [int(v) for v in new_world_size]
        for name, size in (('xy_plane', [X, Y]), ('xz_plane', [X, Z]), ('yz_plane', [Y, Z]), ('x_vec', [X, 1]), ('y_vec', [Y, 1]), ('z_vec', [Z, 1])):
            old = getattr(self, name).data.contiguous()
            setattr(self, name, torch.nn.Parameter(self._as_stored(F.interpolate(old, size=size, mode='bilinear', align_corners=True))))

    def total_variation_add_grad(self, wx, wy, wz, dense_mode):
        """Add the total-variation gradient in place (grid.py:142-154); like the reference, dense_mode is ignored"""
        ps = self.factors()
        for p in ps:
            if p.grad is None:
                p.grad = torch.zeros_like(p, memory_format=torch.preserve_format)
        fn = self.tv_module.tensorf_tv_add_grad if self.tv_module is not None else tensorf_tv_add_grad
        fn(tuple(p.data for p in ps), tuple(p.grad for p in ps), float(wx), float(wy), float(wz))

    def get_dense_grid(self, channels_last=False):
        """the dense [1,C,X,Y,Z] grid (grid.py:156-169), baked by one kernel"""
        f = self._f_vec()
        return tensorf_bake(tuple(p.data for p in self.factors()), None if f is None else f.data, channels_last)

    def extra_repr(self):
        ws = self.world_size.tolist() if torch.is_tensor(self.world_size) else list(self.world_size)
        return f'channels={self.channels}, world_size={ws}, n_comp={self.config["n_comp"]}'


class FourierGrid(torch.nn.Module):
    """Dense voxel grid with optional Fourier levels; mirrors FourierGrid_grid.FourierGrid (same ctor arguments,
    `grid` parameter [P,C,X,Y,Z], `xyz_min` / `xyz_max` buffers, methods), with the lookup, its backward and the
    total-variation gradient on the HIP kernels."""

    def __init__(self, channels, world_size, xyz_min, xyz_max, use_nerf_pos, fourier_freq_num, config=None):
        super().__init__()
        self.channels = channels
        self.world_size = world_size
        self.register_buffer('xyz_min', torch.Tensor(xyz_min))
        self.register_buffer('xyz_max', torch.Tensor(xyz_max))
        # config={'channels_last': True}: store a multi-channel grid as [P][X][Y][Z][C] (torch.channels_last_3d of the same
        # logical [P,C,X,Y,Z] parameter -- state_dicts / checkpoints are unchanged): the HIP lookup, its scatter backward,
        # the TV gradient and the fused TV + Adam pass then touch one 4C-byte run per voxel instead of C planes
        self.channels_last = bool(config.get('channels_last', False)) if isinstance(config, dict) else False
        if use_nerf_pos:
            self.nerf_pos_num_freq = fourier_freq_num
            self.pos_embed_output_dim = 1 + self.nerf_pos_num_freq * 2
            self.grid = torch.nn.Parameter(self._alloc([self.pos_embed_output_dim, channels, *world_size]))
        else:
            self.nerf_pos_num_freq = -1
            self.pos_embed_output_dim = -1
            self.grid = torch.nn.Parameter(self._alloc([1, channels, *world_size]))

    def _alloc(self, shape):
        shape = [int(x) for x in shape]
        if self.channels_last and shape[1] > 1:
            return torch.zeros(shape).contiguous(memory_format=torch.channels_last_3d)
        return torch.zeros(shape)

    def _as_stored(self, t):
        if self.channels_last and t.shape[1] > 1:
            return t.contiguous(memory_format=torch.channels_last_3d)
        return t.contiguous()

    # test hooks: another implementation of the lookup (differentiable, fourier_grid_query's signature) and of the
    # total_variation_cuda module; None = the HIP kernels
    query_fn = None
    tv_module = None

    def forward(self, xyz):
        """xyz [..., 3] world coordinates -> [..., C] (squeezed when C == 1)"""
        q = self.query_fn or GridQuery.apply
        _lib.wait_pending(self.grid)
        return q(self.grid, xyz, self.xyz_min, self.xyz_max, self.nerf_pos_num_freq)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        _lib.wait_pending(self.grid)
        super()._save_to_state_dict(destination, prefix, keep_vars)

    def scale_volume_grid(self, new_world_size):
        _lib.wait_pending(self.grid)
        if self.channels == 0:
            self.grid = torch.nn.Parameter(torch.zeros([1, self.channels, *new_world_size]))
        else:
            self.grid = torch.nn.Parameter(self._as_stored(
                F.interpolate(self.grid.data, size=tuple(int(x) for x in new_world_size), mode='trilinear', align_corners=True)))

    def total_variation_add_grad(self, wx, wy, wz, dense_mode):
        """Add the total-variation gradient in place (total_variation_kernel.cu:14-67)."""
        tv = self.tv_module
        if tv is None:
            from . import total_variation_cuda as tv
        _lib.wait_pending(self.grid)
        tv.total_variation_add_grad(self.grid, self.grid.grad, wx, wy, wz, dense_mode)

    def get_dense_grid(self):
        _lib.wait_pending(self.grid)
        return self.grid

    @torch.no_grad()
    def __isub__(self, val):
        _lib.wait_pending(self.grid)
        self.grid.data -= val
        return self

    def extra_repr(self):
        ws = self.world_size.tolist() if torch.is_tensor(self.world_size) else list(self.world_size)
        return f'channels={self.channels}, world_size={ws}'


class MaskGrid(torch.nn.Module):
    """Occupancy lookup (known free space); same constructor as the reference's MaskGrid (FourierGrid_grid.py:139-158,
    grid.py:205-228): either an explicit boolean `mask` with its bounds, or `path` to a checkpoint whose density grid
    is max-pooled (3x3x3), turned into alpha and thresholded at `mask_cache_thres`."""

    def __init__(self, path=None, mask_cache_thres=None, mask=None, xyz_min=None, xyz_max=None):
        super().__init__()
        if path is not None:
            st = torch.load(path, map_location='cpu', weights_only=False)
            self.mask_cache_thres = mask_cache_thres
            sd, kw = st['model_state_dict'], st['model_kwargs']
            density = F.max_pool3d(sd['density.grid'], kernel_size=3, padding=1, stride=1)
            alpha = 1 - torch.exp(-F.softplus(density + sd['act_shift']) * kw['voxel_size_ratio'])
            mask = (alpha >= self.mask_cache_thres).squeeze(0).squeeze(0)
            xyz_min, xyz_max = torch.Tensor(kw['xyz_min']), torch.Tensor(kw['xyz_max'])
        else:
            mask = mask.bool()
            xyz_min = torch.as_tensor(xyz_min, dtype=torch.float32).cpu()
            xyz_max = torch.as_tensor(xyz_max, dtype=torch.float32).cpu()
        self.register_buffer('mask', mask)
        xyz_len = xyz_max - xyz_min
        scale = (torch.Tensor(list(mask.shape)) - 1) / xyz_len
        self.register_buffer('xyz2ijk_scale', scale)
        self.register_buffer('xyz2ijk_shift', -xyz_min * scale)

    lookup_module = None    # test hook: another implementation of render_utils_cuda; None = the HIP kernels

    @torch.no_grad()
    def forward(self, xyz):
        shape = xyz.shape[:-1]
        ru = self.lookup_module or render_utils_cuda
        out = ru.maskcache_lookup(self.mask, xyz.reshape(-1, 3).contiguous(), self.xyz2ijk_scale, self.xyz2ijk_shift)
        return out.reshape(shape)

    def extra_repr(self):
        return f'mask.shape={list(self.mask.shape)}'
