"""Multi-GPU render: one process per GPU (torch.distributed, backend "nccl" = RCCL over xGMI).

Rays are independent and the grids + rgbnet are read-only at render time, so the
data path is: every rank holds a full replica of the bricks, renders its contiguous ray shard with the
fused kernels, and ONE all-gather exchanges the rendered tiles [rgb(3), depth, alphainv_last] = 20 B/ray.
There is no collective inside the march/shade kernels.

`render_sharded(..., interleave=True)` deals 64-ray tiles round-robin instead of in contiguous ranges: on real
scenes sky and dense regions cluster in the image, and the fused kernels' time per tile follows the survivor
count, so contiguous row bands can be badly unbalanced.

`composite_blocks` is the one-model-per-GPU layout of BASELINE.json configs[4] (Waymo-style blocks): every rank
renders ITS block for ALL rays and one all-reduce(sum) of [R+1,5] merges them.
"""
import torch
import torch.distributed as dist


def shard_bounds(n, world_size, rank, align=64):
    """Contiguous shard [b,e) of n rays for `rank`; shard sizes are multiples of `align` (one wave tile)
    except the last.  Deterministic and identical on every rank."""
    per = -(-n // world_size)
    per = -(-per // align) * align
    b = min(n, rank * per)
    e = min(n, b + per)
    return b, e


def tile_assignment(n, world_size, rank, tile=64, group=1):
    """Indices of the rays of `rank` when the list's 64-ray tiles are dealt round-robin in groups of `group` consecutive tiles
    (group k -> rank k % world_size; group = 1: single tiles).  In render_view's / the bench's 8 x 8 pixel-block ray order a tile
    is one pixel block and consecutive tiles are horizontally adjacent blocks, so group = W / 8 deals whole block ROWS: a rank's rays
    then share grid cells with their horizontal neighbours (what the kernels' cache efficiency rests on) while the shares stay
    balanced over the image; group = 1 gives the finest balance and the least sharing (measured: profiles/r05/scaling_proxy.json)."""
    n_tiles = -(-n // tile)
    n_groups = -(-n_tiles // group)
    mine = torch.arange(rank, max(n_groups, rank), world_size)    # (a rank beyond the last group gets none: arange(r, r) is empty)
    tiles = (mine[:, None] * group + torch.arange(group)[None, :]).reshape(-1)
    idx = (tiles[:, None] * tile + torch.arange(tile)[None, :]).reshape(-1)
    return idx[idx < n]


def render_sharded(renderer_forward, rays_o, rays_d, viewdirs, group=None, interleave=False, deal_group=1, **render_kwargs):
    """Render rays [R,3] split across the process group; every rank returns the full
    {'rgb_marched','depth','alphainv_last'}.  `renderer_forward(o,d,v,**kw)` is FourierGridRenderer.forward
    (or any callable with the reference forward's signature and return keys).  interleave: deal tiles round-robin in groups of
    `deal_group` consecutive 64-ray tiles (tile_assignment) instead of contiguous ranges."""
    ws = dist.get_world_size(group) if dist.is_initialized() else 1
    rk = dist.get_rank(group) if dist.is_initialized() else 0
    R = rays_o.shape[0]
    kw = dict(render_kwargs)
    kw["render_depth"] = True
    if interleave and ws > 1:
        idx = tile_assignment(R, ws, rk, group=deal_group).to(rays_o.device)
        n_mine = idx.numel()
        per = tile_assignment(R, ws, 0, group=deal_group).numel()      # rank 0 always holds the largest share
        o_, d_, v_ = rays_o[idx].contiguous(), rays_d[idx].contiguous(), viewdirs[idx].contiguous()
    else:
        b, e = shard_bounds(R, ws, rk)
        n_mine = e - b
        per = shard_bounds(R, ws, 0)[1]
        o_, d_, v_ = rays_o[b:e].contiguous(), rays_d[b:e].contiguous(), viewdirs[b:e].contiguous()
    tile = torch.zeros(per, 5, dtype=torch.float32, device=rays_o.device)
    if n_mine > 0:
        out = renderer_forward(o_, d_, v_, **kw)
        tile[:n_mine, 0:3] = out["rgb_marched"]
        tile[:n_mine, 3] = out["depth"]
        tile[:n_mine, 4] = out["alphainv_last"]
    if ws > 1:
        full = torch.empty(ws * per, 5, dtype=torch.float32, device=rays_o.device)
        dist.all_gather_into_tensor(full, tile, group=group)
        if interleave:
            # undo the deal: rank r's rows are its tiles r, r+ws, ... in order
            res = torch.empty(R, 5, dtype=torch.float32, device=rays_o.device)
            for r in range(ws):
                ir = tile_assignment(R, ws, r, group=deal_group).to(rays_o.device)
                res[ir] = full[r * per: r * per + ir.numel()]
            full = res
    else:
        full = tile
    full = full[:R]
    return {"rgb_marched": full[:, 0:3].contiguous(), "depth": full[:, 3].contiguous(),
            "alphainv_last": full[:, 4].contiguous()}



# ---------------------------------------------------------------------------------------------------------------------------
# The frame pipeline: a view list over the process group, for every renderer of the package
# ---------------------------------------------------------------------------------------------------------------------------
_PLANS = {}
DEALS = ("bands", "rows", "tiles")


class FramePlan:
    """Who renders which pixel of an H x W frame split over `world` ranks, and where a pixel's result lies in the all-gathered
    buffer [world*per,5] -- pure host arithmetic, one object per key (FramePlan(...) returns the cached one).

    Ray order: the 8 x 8 pixel-block order of fourier_render.pixel_tile_order when H and W are multiples of 8 (`tile8`), else image
    order (q = y*W + x).  The split of the R = H*W ray positions: deal = 'bands' -> contiguous 64-aligned ranges (shard_bounds);
    'tiles' -> 64-ray tiles dealt singly; 'rows' -> in groups of W/8 tiles, whole block rows of the image; deal_group > 0 -> in
    groups of that many tiles whatever `deal` says (tile_assignment; `deal_group` of the plan is 0 for bands).
    `per` = rows of a rank's block of the gathered buffer (rank 0 holds the largest share), `px(rank)` = the flat pixel indices
    y*W + x a rank renders, in its ray order.  `source_row` is the closed form that ugrid_frame_assemble evaluates per pixel;
    `src_index` is the same table built the slow way, rank by rank, for the tests and the CPU path."""

    def __new__(cls, H, W, world, deal="bands", deal_group=0, tile=8):
        H, W, world, dg, tile = int(H), int(W), int(world), int(deal_group or 0), int(tile)
        if deal not in DEALS:
            raise ValueError("deal must be one of %s (got %r)" % (DEALS, deal))
        if H < 1 or W < 1 or world < 1 or dg < 0:
            raise ValueError("FramePlan: H, W, world >= 1 and deal_group >= 0 expected (got %d, %d, %d, %d)" % (H, W, world, dg))
        if dg == 0 and deal != "bands":
            dg = max(1, W // 8) if deal == "rows" else 1
        key = (H, W, world, dg, tile)
        plan = _PLANS.get(key)
        if plan is None:
            if len(_PLANS) > 64:
                _PLANS.clear()
            plan = _PLANS[key] = object.__new__(cls)
            plan._build(H, W, world, dg, tile)
        return plan

    def _build(self, H, W, world, dg, tile):
        from .fourier_render import _morton_ok, pixel_tile_order
        self.H, self.W, self.R, self.world, self.deal_group = H, W, H * W, world, dg
        # (the kernel's block order is the Z-order one: with UGRID_TILE_MORTON=0 a plan stays in image order)
        self.tile8 = tile == 8 and H % 8 == 0 and W % 8 == 0 and _morton_ok(8)
        self.order = pixel_tile_order(H, W, torch.device("cpu"), 8).clone() if self.tile8 else None
        self.per = tile_assignment(self.R, world, 0, group=dg).numel() if dg else shard_bounds(self.R, world, 0)[1]
        self._src = None
        self._px = {}

    def positions(self, rank):
        """ray positions q of `rank`, ascending within a tile, in the order the rank renders and sends them"""
        if self.deal_group:
            return tile_assignment(self.R, self.world, rank, group=self.deal_group).to(torch.int64)
        b, e = shard_bounds(self.R, self.world, rank)
        return torch.arange(b, e, dtype=torch.int64)

    def px(self, rank, device=None):
        """flat pixel indices of `rank` (int64, on `device`; default: the host), cached"""
        key = (int(rank), str(device))
        t = self._px.get(key)
        if t is None:
            q = self.positions(rank)
            t = (q if self.order is None else self.order[q]).contiguous()
            if device is not None:
                t = t.to(device)
            self._px[key] = t
        return t

    def source_row(self, pixel):
        """row of the gathered buffer that holds flat pixel index `pixel` (int or int64 tensor): ugrid_frame_assemble's formula"""
        p = torch.as_tensor(pixel, dtype=torch.int64)
        q = p
        if self.tile8:
            y, x = p // self.W, p % self.W
            lane = ((y & 4) << 3) | ((x & 4) << 2) | ((y & 2) << 2) | ((x & 2) << 1) | ((y & 1) << 1) | (x & 1)
            q = ((y >> 3) * (self.W >> 3) + (x >> 3)) * 64 + lane
        dg, ws, per = self.deal_group, self.world, self.per
        if dg == 0:
            rank, off = q // per, q % per
        else:
            t = q // 64
            g = t // dg
            rank, off = g % ws, ((g // ws) * dg + t % dg) * 64 + q % 64
        return rank * per + off

    def src_index(self):
        """the table of source_row over all pixels, int64 [R], built from every rank's own list (cached)"""
        if self._src is None:
            pix_of_row = torch.full((self.world * self.per,), -1, dtype=torch.int64)
            for r in range(self.world):
                pr = self.px(r)
                pix_of_row[r * self.per: r * self.per + pr.numel()] = pr
            rows = torch.nonzero(pix_of_row >= 0).reshape(-1)
            src = torch.full((self.R,), -1, dtype=torch.int64)
            src[pix_of_row[rows]] = rows
            self._src = src
        return self._src


def _stream_of(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def frame_pack(rgb, depth, last, per):
    """A rank's send tile [per,5]: rows 0..n = rgb(3), depth, alphainv_last of its n rays, rows n..per zero (n = 0, three empty tensors, is
    legal: a zero tile).  Device tensors: ugrid_frame_pack, one launch; host tensors: the torch composition (tests of the
    exchange logic)."""
    n = int(depth.shape[0])
    out = torch.empty(per, 5, dtype=torch.float32, device=depth.device)
    if not depth.is_cuda:
        out.zero_()
        out[:n, 0:3], out[:n, 3], out[:n, 4] = rgb, depth, last
        return out
    from . import _lib
    rgb, depth, last = rgb.contiguous(), depth.contiguous(), last.contiguous()
    _lib.require_f32(("rgb", rgb), ("depth", depth), ("last", last))
    with _lib.guard(depth.device):
        _lib.check(_lib.load().ugrid_frame_pack(_lib.ptr(rgb) if n else None, _lib.ptr(depth) if n else None, _lib.ptr(last) if n else None,
                                                n, per, _lib.ptr(out), _stream_of(depth.device)), "frame_pack")
    return out


def frame_assemble(plan, gathered=None, rgb=None, depth=None, last=None):
    """The packed frame [H*W,5] in image order from the gathered buffer [world*per,5] of `plan`, or (gathered None) from the three
    per-ray arrays of a whole frame in the plan's ray order.  Device tensors: ugrid_frame_assemble, one launch, no index table;
    host tensors: index_select with plan.src_index()."""
    src = gathered if gathered is not None else depth
    if not src.is_cuda:
        if gathered is None:      # (whole frame in ray order: the rows of a one-rank plan)
            gathered = torch.cat([rgb.reshape(-1, 3), depth.reshape(-1, 1), last.reshape(-1, 1)], dim=1)
            plan = FramePlan(plan.H, plan.W, 1, tile=8 if plan.tile8 else 0)
        return torch.index_select(gathered, 0, plan.src_index())
    from . import _lib
    out = torch.empty(plan.R, 5, dtype=torch.float32, device=src.device)
    with _lib.guard(src.device):
        if gathered is not None:
            assert gathered.is_contiguous() and gathered.dtype == torch.float32 and gathered.numel() == plan.world * plan.per * 5
            err = _lib.load().ugrid_frame_assemble(_lib.ptr(gathered), None, None, None, plan.H, plan.W, plan.world, plan.per,
                                                   plan.deal_group, int(plan.tile8), _lib.ptr(out), _stream_of(src.device))
        else:
            rgb, depth, last = rgb.contiguous(), depth.contiguous(), last.contiguous()
            _lib.require_f32(("rgb", rgb), ("depth", depth), ("last", last))
            assert depth.numel() == plan.R and last.numel() == plan.R and rgb.numel() == 3 * plan.R
            err = _lib.load().ugrid_frame_assemble(None, _lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(last), plan.H, plan.W, 1, plan.R, 0,
                                                   int(plan.tile8), _lib.ptr(out), _stream_of(src.device))
        _lib.check(err, "frame_assemble")
    return out


class FramePipeline:
    """A view list rendered over a process group, for FourierGridRenderer (and its composed twin) and the BoundedRenderer family
    (DirectVoxGORenderer, DirectContractedVoxGORenderer, DirectMPIGORenderer -- NDC rays for the last).

    submit(H, W, K, c2w, **kw) issues one view on the CURRENT stream: rays of this rank's pixels only (FramePlan.px), one render
    pass, ugrid_frame_pack, and an asynchronous all_gather_into_tensor into one of two gathered buffers.  Just before the collective
    is issued the PREVIOUS view is completed -- a stream-level wait for its collective, then ugrid_frame_assemble -- so a view's
    exchange runs beside the next view's render.  submit returns the frame it completed (a packed [H*W,5] device tensor in image
    order: rgb(3), depth, alphainv_last) or None; flush() completes the last one.  Frames come back in submission order, each once.
    kw: stepsize, inverse_y, flip_x, flip_y, and for the bounded family near / far / bg (what run_render passes on).

    Order rules (every one is needed; bench.py's FrameBench keeps the same):
      * a gathered buffer goes into a new collective only after the issuing stream has waited on the event recorded behind the
        assembly that read it (with views on several streams that assembly ran on another stream);
      * a send tile is referenced until its collective has been waited for, and handed to the waiting stream before it is dropped;
      * every rank issues its collectives in view order, a rank without rays included (it sends a zero tile);
      * frame sizes may change from view to view: a plan per size, the buffers regrown.
    Without a process group, or with one rank, there is no exchange: submit returns the view's own frame, assembled from the three
    per-ray arrays.  On host tensors (gloo tests with a stand-in renderer) torch composes what the two kernels do."""

    def __init__(self, model, group=None, deal="bands", deal_group=0):
        on = dist.is_available() and dist.is_initialized()
        self.model, self.group = model, group
        self.device = torch.device(model.device)
        self.world = dist.get_world_size(group) if on else 1
        self.rank = dist.get_rank(group) if on else 0
        self.deal, self.deal_group = deal or "bands", int(deal_group or 0)
        self.ndc = bool(getattr(model, "ndc", False))
        self._gathered = [None, None]
        self._assembled_ev = [None, None]
        self._inflight = None
        self._n = 0

    def _render(self, block_order, o, d, v, kw):
        m = self.model
        if hasattr(m, "fused_supported"):          # BoundedRenderer family: render_rays, as render_view_of calls it
            rk = {k: kw[k] for k in ("near", "far", "stepsize", "bg") if k in kw}
            if m.fused_supported():                # (the composed forward takes no ray_order)
                ray_order = "coherent" if block_order else m.ray_order
                if ray_order is not None:
                    rk["ray_order"] = ray_order
            return m.render_rays(o, d, v, render_depth=True, **rk)
        return m.forward(o, d, v, stepsize=kw["stepsize"], ray_order="coherent" if block_order else "auto", render_depth=True)

    def _rays(self, H, W, K, c2w, px, kw):
        from .fourier_render import get_rays_of_pixel_index
        return get_rays_of_pixel_index(H, W, K, c2w, px, inverse_y=bool(kw.get("inverse_y", False)), flip_x=bool(kw.get("flip_x", False)),
                                       flip_y=bool(kw.get("flip_y", False)), ndc=self.ndc)

    def render_local(self, H, W, K, c2w, **kw):
        """one whole view on this device, no exchange: the packed frame [H*W,5]"""
        from .fourier_render import get_rays_of_a_view, pixel_tile_order
        plan = FramePlan(H, W, 1)
        dev = self.device
        c2w = torch.as_tensor(c2w, dtype=torch.float32).to(dev)
        if plan.tile8:
            o, d, v = self._rays(H, W, K, c2w, pixel_tile_order(H, W, dev, 8), kw)
        else:
            o, d, v = get_rays_of_a_view(H, W, K, c2w, inverse_y=bool(kw.get("inverse_y", False)), flip_x=bool(kw.get("flip_x", False)),
                                         flip_y=bool(kw.get("flip_y", False)), ndc=self.ndc)
            o, d, v = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), v.reshape(-1, 3).contiguous()
        out = self._render(plan.tile8, o, d, v, kw)
        return frame_assemble(plan, rgb=out["rgb_marched"], depth=out["depth"], last=out["alphainv_last"])

    def submit(self, H, W, K, c2w, **kw):
        if self.world == 1:
            return self.render_local(H, W, K, c2w, **kw)
        dev = self.device
        cuda = dev.type == "cuda"
        plan = FramePlan(H, W, self.world, self.deal, self.deal_group)
        c2w = torch.as_tensor(c2w, dtype=torch.float32).to(dev)
        px = plan.px(self.rank, dev)
        if px.numel() > 0:
            o, d, v = self._rays(H, W, K, c2w, px, kw)
            out = self._render(plan.tile8, o, d, v, kw)
            rgb, depth, last = out["rgb_marched"], out["depth"], out["alphainv_last"]
        else:                                       # an empty share: a zero tile, and the rank still takes part in the collective
            rgb, depth, last = torch.empty(0, 3, device=dev), torch.empty(0, device=dev), torch.empty(0, device=dev)
        tile = frame_pack(rgb, depth, last, plan.per)
        done = self._complete()                     # the previous view: wait for its exchange, assemble it beside this view's
        k = self._n & 1
        if cuda and self._assembled_ev[k] is not None:      # (the assembly that last read gathered[k] may have run on another stream)
            torch.cuda.current_stream(dev).wait_event(self._assembled_ev[k])
        need = self.world * plan.per * 5
        buf = self._gathered[k]
        if buf is None or buf.numel() < need:
            if cuda and buf is not None:
                buf.record_stream(torch.cuda.current_stream(dev))
            buf = self._gathered[k] = torch.empty(need, dtype=torch.float32, device=dev)
        full = buf[:need].view(self.world * plan.per, 5)
        work = dist.all_gather_into_tensor(full, tile, group=self.group, async_op=True)
        self._inflight = {"work": work, "tile": tile, "full": full, "plan": plan, "k": k}
        self._n += 1
        return done

    def _complete(self):
        fl, self._inflight = self._inflight, None
        if fl is None:
            return None
        fl["work"].wait()                           # stream-level for a device collective
        frame = frame_assemble(fl["plan"], gathered=fl["full"])
        if self.device.type == "cuda":
            st = torch.cuda.current_stream(self.device)
            self._assembled_ev[fl["k"]] = st.record_event()
            fl["tile"].record_stream(st)            # (allocated on the stream that sent it, released behind this stream's wait)
        return frame

    def flush(self):
        """complete the last submitted view: its frame, or None when nothing is in flight"""
        return self._complete()


INVISIBLE_SCALE = 2.0 ** -60   # weight factor of a block that fails the visibility test (see composite_blocks)


def composite_blocks(renderer_forward, rays_o, rays_d, viewdirs, cam_origin, block_centroid, p=4.0, min_opacity=0.05,
                     group=None, ref_distance=None, all_centroids=None, **render_kwargs):
    """One block model per rank, the same rays on every rank, ONE all-reduce(sum) of [R+1,5] fp32, no host sync.

    The reference's FourierGrid path never composites blocks (it renders each block's own image subset,
    run_render.py:146-207); the only merging rule in the repository is the legacy Block-NeRF evaluation
    (eval_block_nerf.py:95-133,215-225): keep a block if its mean visibility exceeds 0.05, weight it by the inverse
    camera-to-centroid distance to the power p (IDW_Power = 4), normalise the weights, blend the images.  This
    function applies that rule to the fused renderer's float outputs: visibility of a block := its mean
    accumulated opacity 1 - alphainv_last over the rays (the FourierGrid model has no visibility network), weight
    w_b = |cam_origin - block_centroid|^-p if visible, result = sum_b w_b * [rgb, depth, alphainv_last] / sum_b w_b.

    Everything stays on the device: the visibility test is a device-side comparison folded into w_b, and row R of the
    reduced buffer carries (sum_b w_b, number of visible blocks, 0, 0, 0), so one collective returns both the numerators
    and the normaliser.  A block that FAILS the test is not dropped but scaled by 2^-60: next to any visible block its
    contribution is below fp32 resolution (the blend is bit-identical to excluding it unless its distance weight exceeds
    the visible ones' by > 10^10), and when NO block is visible -- the reference skips such a frame
    (eval_block_nerf.py:225-226) -- the common factor cancels and the frame is the inverse-distance blend of all blocks,
    without a second collective or a host decision.

    Scale of the distance weight.  Only the RATIOS of the w_b matter, and |cam - centroid|^-p itself is not a safe fp32 quantity:
    un-centred city-scale coordinates put cameras 1e4 ... 1e5 units from the centroids (1e-20, and 1e-20 * 2^-60 is denormal), a
    camera inside a block makes it huge.  The weight is therefore formed in RELATIVE space, (|cam - centroid| / ref)^-p in float64
    with ref = the distance of the NEAREST block, so the nearest block weighs exactly 1 and every other block <= 1 whatever the
    units; only the far end is clamped, at 2^-60 (a block 2^15 times farther than the nearest at p = 4: 36 binary orders below
    fp32's resolution next to it -- the clamp keeps w_b * 2^-60 a normal number, it never changes a ratio that could be seen).
    `ref` must be the same on every rank:
      * `all_centroids` (the centroids of ALL blocks, e.g. from the scene's block table): every rank computes the minimum itself --
        the function stays at ONE collective;
      * or `ref_distance` (any agreed positive number, e.g. the block spacing; weights may then exceed 1);
      * neither: one extra 8-byte all-reduce(MIN) of the rank's own distance agrees on it (device-side, no host sync).
    (Round 4 clamped the ABSOLUTE weight into [2^-40, 2^40]: with the default ref = 1 every camera further than 1024 units from
    every centroid got the same weight and the blend silently became a plain average -- ADVICE r4.)
    Returned `block_weight` is this rank's NORMALISED weight as a 0-d device tensor (w_b / sum_b w_b), `visible_blocks` the number
    of blocks that passed the test."""
    ws = dist.get_world_size(group) if dist.is_initialized() else 1
    kw = dict(render_kwargs)
    kw["render_depth"] = True
    out = renderer_forward(rays_o, rays_d, viewdirs, **kw)
    R = rays_o.shape[0]
    dev = rays_o.device
    cam64 = torch.as_tensor(cam_origin, dtype=torch.float64).reshape(3).cpu()
    d_own = (cam64 - torch.as_tensor(block_centroid, dtype=torch.float64).reshape(3).cpu()).norm()      # host arithmetic
    if ref_distance is not None:
        ref = torch.as_tensor(float(ref_distance), dtype=torch.float64)
    elif all_centroids is not None:
        cents = torch.stack([torch.as_tensor(c, dtype=torch.float64).reshape(3).cpu() for c in all_centroids])
        ref = (cents - cam64[None]).norm(dim=1).min()
    elif ws > 1:
        ref = d_own.to(dev).reshape(1).clone()
        dist.all_reduce(ref, op=dist.ReduceOp.MIN, group=group)          # 8 bytes; stays on the device
        ref = ref[0]
    else:
        ref = d_own
    rel = d_own.to(ref.device) / ref.clamp_min(1e-300)
    dw = (rel ** (-float(p))).clamp(2.0 ** -60, 2.0 ** 60).to(device=dev, dtype=torch.float32)  # one scalar upload at most
    # (upper end: only an explicit ref_distance can put a block above 1 -- a camera sitting ON a centroid must not produce inf)
    opacity = (1.0 - out["alphainv_last"]).mean() if R > 0 else torch.zeros((), device=dev)
    visible = (opacity > min_opacity).to(torch.float32)                  # 0-d device tensor
    w = dw * (visible + (1.0 - visible) * INVISIBLE_SCALE)
    acc = torch.empty(R + 1, 5, dtype=torch.float32, device=dev)
    acc[:R, 0:3] = out["rgb_marched"] * w
    acc[:R, 3] = out["depth"] * w
    acc[:R, 4] = out["alphainv_last"] * w
    acc[R, 0] = w
    acc[R, 1] = visible
    acc[R, 2:] = 0.0
    if ws > 1:
        dist.all_reduce(acc, group=group)
    norm = acc[R, 0].clamp_min(2.0 ** -120)
    blended = acc[:R] / norm
    return {"rgb_marched": blended[:, 0:3].contiguous(), "depth": blended[:, 3].contiguous(),
            "alphainv_last": blended[:, 4].contiguous(), "block_weight": w / norm, "visible_blocks": acc[R, 1]}
