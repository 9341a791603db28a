"""Frame loop of the render driver: the MI355X counterpart of
run_render.render_viewpoints (/root/reference/FourierGrid/run_render.py:14-114).

The reference generates rays on the host, renders 8192-ray chunks through a dict-per-chunk loop, concatenates, and
calls `.cpu().numpy()` three times per frame (a blocking device sync each).  Here a frame is: rays generated on the
device, ONE fused march + shade pass over all H*W rays (sharded over the process group when one is initialised,
dist.render_sharded), and ONE asynchronous device-to-host copy of the packed [H,W,5] result into pinned memory on
a side stream, overlapped with the next frame's render.  The views of a list are independent frames: consecutive ones are
issued on two alternating streams, each with a work list of its own (frames_in_flight = 2), so that the march of view k + 1
runs beside the shade of view k -- whole frames at 1080p: 8.8 -> 8.4 ms per view on white-noise grids, 14.0 -> 12.4 ms on
a trained-like truck-shaped scene, every frame bit-identical (profiles/r06/frame_pair_n1.txt).  Same return values as the
reference: numpy arrays rgbs [N,H,W,3], depths [N,H,W,1], bgmaps [N,H,W,1] (+ PSNRs when ground truth is given; + SSIMs with
eval_ssim, the reference's --eval_ssim: scored on the device by metrics.frame_metrics, on the stream that rendered the view).

With a process group of more than one rank every renderer goes through dist.FramePipeline: a rank generates and renders its own
pixels only, the tiles are exchanged asynchronously, and view k is assembled (one kernel, ugrid_frame_assemble) while view k + 1
renders.  In a single process the same kernel puts the frame together from the per-ray arrays (FUSED_ASSEMBLY).

render_video runs the same loop (_FrameLoop) and returns the frames as the uint8 arrays a video writer takes -- rgb, and the
reference's two depth videos -- made on the device by the ops of video.py: 3 bytes a pixel come to the host instead of 20."""
import numpy as np
import torch

# single process: assemble the packed frame with ugrid_frame_assemble from the three per-ray arrays (one launch) instead of three
# un-tile permute-copies and a torch.cat (False: that epilogue).  The frames are bit-identical either way.
FUSED_ASSEMBLY = True


@torch.no_grad()
def render_viewpoints(model, render_poses, HW, Ks, render_kwargs, gt_imgs=None, render_factor=0,
                      flip_x=False, flip_y=False, group=None, verbose=False, frames_in_flight=None, eval_ssim=False, deal=None, deal_group=0):
    """model: FourierGridRenderer, or a DirectVoxGORenderer / DirectContractedVoxGORenderer (their render_view takes the
    reference's render_kwargs 'near', 'far', 'bg' as well); render_poses [N,3or4,4] camera-to-world; HW [N,2]; Ks [N,3,3];
    render_kwargs: needs 'stepsize', may carry 'inverse_y' (the keys run_render.py passes; others are ignored).
    frames_in_flight (default: the model's own `frames_in_flight` attribute, else 2): n >= 2 = consecutive views take n streams and
    n work lists in turn (renderers with use_workspace_slot; every further work list costs up to 8.4 GB at 1080p x 256 samples),
    1 = one stream.  2 is within 2 % of the best for 1080p frames; a view that leaves most of the chip idle gains from 4
    (DirectVoxGO, 800 x 800: 1.88 / 1.03 / 0.78 ms per view at 1 / 2 / 4; profiles/r06/frames_in_flight_sweep.txt).
    eval_ssim (needs gt_imgs and render_factor == 0, ValueError otherwise -- the reference skips the metric silently): view i's
    ground truth is uploaded on the stream that renders view i and ugrid_frame_metrics runs there right behind the render, reading
    the rgb columns of the packed result in place; the sums of all views land in one [N,2] device tensor that is read once, after the
    loop.  The ground truth comes from pageable host memory, so each upload blocks the HOST for the duration of the copy (the
    device keeps rendering the view queued just before); one ground-truth buffer and one scratch per view in flight.  With a
    process group every rank scores the assembled frame.
    deal / deal_group (process group of more than one rank): how dist.FramePlan splits a frame -- None or 'bands' = contiguous ranges,
    'tiles' = 64-ray tiles dealt singly, 'rows' = whole block rows of the image, deal_group > 0 = groups of that many tiles.  View i is
    then completed (exchange awaited, assembled, scored, copied out) on the stream of view i + 1; every rank returns every frame.
    Returns (rgbs, depths, bgmaps), (rgbs, depths, bgmaps, psnrs) when gt_imgs is given, or (rgbs, depths, bgmaps, psnrs, ssims)
    with eval_ssim: ssims[i] is a Python float, the mean of view i's SSIM map (= metrics.rgb_ssim(rgbs[i], gt_imgs[i], 1)).
    psnrs is computed on the host from the returned frames in every case."""
    if eval_ssim:
        if gt_imgs is None:
            raise ValueError("eval_ssim needs gt_imgs")
        if render_factor != 0:
            raise ValueError("eval_ssim needs render_factor == 0 (the ground truth has the full frame's size)")
        if len(gt_imgs) != len(render_poses):
            raise ValueError("eval_ssim: %d ground-truth images for %d views" % (len(gt_imgs), len(render_poses)))
    assert len(render_poses) == len(HW) and len(HW) == len(Ks)
    HW = np.asarray(HW).copy()
    Ks = np.asarray(Ks, dtype=np.float64).copy()
    if render_factor != 0:                                    # run_render.py:22-26
        HW = (HW / render_factor).astype(int)
        Ks[:, :2, :3] /= render_factor
    if eval_ssim:
        for i in range(len(HW)):
            if tuple(np.shape(gt_imgs[i])) != (int(HW[i][0]), int(HW[i][1]), 3):
                raise ValueError("gt_imgs[%d] is %s, view %d is %d x %d" % (i, tuple(np.shape(gt_imgs[i])), i, HW[i][0], HW[i][1]))
            if min(int(HW[i][0]), int(HW[i][1])) < 11:
                raise ValueError("eval_ssim: view %d is %d x %d, the 11-tap SSIM window needs 11 x 11" % (i, HW[i][0], HW[i][1]))
    loop = _FrameLoop(model, len(render_poses), group, frames_in_flight, deal, deal_group)
    dev, copy_stream = loop.dev, loop.copy_stream
    n = len(render_poses)
    n_slots = loop.n_slots
    host = [None] * n_slots       # pinned buffers (one per view in flight), re-allocated when the frame size changes
    done = [None] * n_slots
    frames = []
    if eval_ssim:
        from . import metrics
        sums = torch.empty((n, 2), dtype=torch.float64, device=dev)   # (written on the views' streams; the caller's stream joins them before the read)
        gt_dev = [None] * n_slots   # per view in flight: ground truth [>= H*W*3] and the kernel's scratch, both allocated on the
        gt_ws = [None] * n_slots    # slot's stream and re-used there in stream order
        gt_src = [None] * n       # the host arrays being uploaded, held until their view is drained

    def drain(slot, H, W, view):
        done[slot].synchronize()
        a = host[slot][: H * W * 5].numpy().reshape(H, W, 5).copy()
        frames.append(a)
        if eval_ssim:
            gt_src[view] = None

    pending = []                  # (slot, H, W) of copies in flight, oldest first

    def finish(i, packed, stream, gslot):
        """view i's packed frame, produced on `stream` (the current one): score it there, queue its copy to the host"""
        H, W = int(HW[i][0]), int(HW[i][1])
        if eval_ssim:
            g = np.ascontiguousarray(np.asarray(gt_imgs[i]), dtype=np.float32)
            need = metrics.workspace_bytes(H, W)
            if gt_dev[gslot] is None or gt_dev[gslot].numel() < g.size:
                gt_dev[gslot] = torch.empty(g.size, dtype=torch.float32, device=dev)
            if gt_ws[gslot] is None or gt_ws[gslot].numel() < need:
                gt_ws[gslot] = torch.empty(need, dtype=torch.uint8, device=dev)
            gt_src[i] = g
            gt_dev[gslot][: g.size].copy_(torch.from_numpy(g).reshape(-1), non_blocking=True)
            metrics.frame_metrics(packed.view(H * W, 5), gt_dev[gslot][: g.size].view(H * W, 3), max_val=1.0, out=sums[i],
                                  H=H, W=W, ws=gt_ws[gslot])
        ready = stream.record_event()       # (behind the metric: a drained slot's ground truth and scratch are free again)
        slot = i % n_slots
        if len(pending) == n_slots:     # the buffer about to be re-used must have been read out
            drain(*pending.pop(0))
        if host[slot] is None or host[slot].numel() < packed.numel():
            host[slot] = torch.empty(packed.numel(), dtype=torch.float32, pin_memory=True)
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(ready)
            host[slot][: packed.numel()].copy_(packed, non_blocking=True)
            packed.record_stream(copy_stream)
            done[slot] = copy_stream.record_event()
        pending.append((slot, H, W, i))
        if verbose:
            print("render_viewpoints: frame %d/%d queued (%dx%d)" % (i + 1, n, W, H))

    loop.run(render_poses, HW, Ks, render_kwargs, flip_x, flip_y, finish)
    while pending:
        drain(*pending.pop(0))
    loop.join()
    res = _stack(frames, gt_imgs, render_factor, n)
    if not eval_ssim:
        return res
    host_sums = sums.cpu().numpy()        # the one read of the metric (the caller's stream has joined every view's stream above)
    ssims = [metrics.mean_ssim(host_sums[i, 1], int(HW[i][0]), int(HW[i][1])) for i in range(n)]
    return res + (ssims,)


@torch.no_grad()
def render_video(model, render_poses, HW, Ks, render_kwargs, render_factor=0, flip_x=False, flip_y=False, render_video_flipy=False,
                 render_video_rot90=0, depth=None, colormap=None, q=(5, 95), bg_thres=0.1, group=None, frames_in_flight=None,
                 deal=None, deal_group=0, mem_get_info=None):
    """The frames of a video as the bytes a video writer takes, made on the device (video.py, csrc/ugrid_video.hip): the same view
    loop as render_viewpoints, but behind every render ugrid_frame_rgb8 turns the packed frame into uint8 [H',W',3] on the view's
    stream -- oriented by render_video_flipy / render_video_rot90 as run_render.py:93-103 orients the float frames -- and 3 bytes a
    pixel (not 20) go to the host through a pinned ring.  model, render_poses, HW, Ks, render_kwargs, render_factor, flip_x, flip_y,
    group, frames_in_flight, deal, deal_group: as render_viewpoints.
    depth: None; 'max' = utils.to8b(1 - depths / np.max(depths)) (run_render.py:284), uint8 [N,H',W',1]; 'percentile' = the rainbow
    depth video of run_render.py:308-315, uint8 [N,H',W',3]: depths_vis = depths*(1 - bgmaps) + bgmaps, dmin / dmax = its q-th
    percentiles over the pixels of ALL frames with bgmaps < bg_thres, colours from `colormap` (uint8 [256,3]; default
    video.rainbow_table()).  Both keep 8 bytes a pixel (depth, alphainv_last) of every view in ONE device buffer, whose size is known
    before the loop: RuntimeError naming the byte counts when mem_get_info(device) (default torch.cuda.mem_get_info) reports less
    free.  After the loop: one host read (the maximum, or the count and four order statistics), then one conversion launch per view.
    Returns (rgb8, depth8, info): arrays [N,H',W',C], or lists of [H',W',C] arrays when the views differ in size; depth8 is None
    without a depth mode; info = {} / {'dmax'} / {'dmin', 'dmax', 'n_masked'}.  'percentile' with no pixel under the threshold:
    depth8 None, n_masked 0 (the reference prints a warning and writes no depth video)."""
    from . import video
    if depth not in (None, "max", "percentile"):
        raise ValueError("depth: None, 'max' or 'percentile' expected (got %r)" % (depth,))
    assert len(render_poses) == len(HW) and len(HW) == len(Ks)
    HW = np.asarray(HW).copy()
    Ks = np.asarray(Ks, dtype=np.float64).copy()
    if render_factor != 0:                                    # run_render.py:22-26
        HW = (HW / render_factor).astype(int)
        Ks[:, :2, :3] /= render_factor
    n = len(render_poses)
    flipy, rot = bool(render_video_flipy), int(render_video_rot90)
    sizes = [(int(h), int(w)) for h, w in HW]
    out_sizes = [video.out_shape(h, w, rot) for h, w in sizes]
    same = len(set(out_sizes)) <= 1
    loop = _FrameLoop(model, n, group, frames_in_flight, deal, deal_group)
    dev, copy_stream, n_slots = loop.dev, loop.copy_stream, loop.n_slots
    offs = np.concatenate([[0], np.cumsum([h * w for h, w in sizes])]).astype(np.int64)      # view i's pixels in the db buffer
    db_all = dmax_word = None
    if depth is not None:
        need = int(offs[-1]) * 8
        free = int((mem_get_info or torch.cuda.mem_get_info)(dev)[0])
        if need > free:
            raise RuntimeError("render_video(depth=%r) keeps (depth, alphainv_last) of %d views = %d pixels on the device: %d bytes needed "
                               "on %s, %d bytes are free" % (depth, n, int(offs[-1]), need, dev, free))
        db_all = torch.empty((int(offs[-1]), 2), dtype=torch.float32, device=dev)      # (written on the views' streams, read after join())
        if depth == "max":
            dmax_word = torch.zeros(1, dtype=torch.int32, device=dev)
    rgb8 = np.empty((n,) + out_sizes[0] + (3,), dtype=np.uint8) if same and n else [None] * n
    host = [None] * n_slots       # pinned byte buffers, one per copy in flight
    done = [None] * n_slots
    pending = []

    def drain(slot, view):
        done[slot].synchronize()
        Ho, Wo = out_sizes[view]
        src = host[slot][: Ho * Wo * 3].numpy().reshape(Ho, Wo, 3)
        if same:
            rgb8[view][...] = src
        else:
            rgb8[view] = src.copy()

    def finish(i, packed, stream, gslot):
        H, W = sizes[i]
        db = db_all[int(offs[i]): int(offs[i + 1])] if db_all is not None else None
        frame8 = video.frame_rgb8(packed.view(H * W, 5), H, W, flipy, rot, db=db, dmax=dmax_word).reshape(-1)
        ready = stream.record_event()
        slot = i % n_slots
        if len(pending) == n_slots:
            drain(*pending.pop(0))
        if host[slot] is None or host[slot].numel() < frame8.numel():
            host[slot] = torch.empty(frame8.numel(), dtype=torch.uint8, pin_memory=True)
        with torch.cuda.stream(copy_stream):
            copy_stream.wait_event(ready)
            host[slot][: frame8.numel()].copy_(frame8, non_blocking=True)
            frame8.record_stream(copy_stream)
            done[slot] = copy_stream.record_event()
        pending.append((slot, i))

    loop.run(render_poses, HW, Ks, render_kwargs, flip_x, flip_y, finish)
    while pending:
        drain(*pending.pop(0))
    loop.join()
    if depth is None:
        return rgb8, None, {}
    # ---- the depth video, on the caller's stream (it has joined every view's stream)
    if depth == "max":
        dmax = float(video.depth_key_to_float(dmax_word.item())) if n else 0.0
        info, C = {"dmax": dmax}, 1
    else:
        def select(ranks):
            return video.depthvis_select(db_all, ranks, bg_thres)[1]
        cnt = video.depthvis_select(db_all, (), bg_thres)[0]
        if cnt == 0:
            return rgb8, None, {"dmin": None, "dmax": None, "n_masked": 0}
        dmin, dmax = (float(v) for v in video.percentile_from_order_stats(cnt, list(q), select))
        info, C = {"dmin": dmin, "dmax": dmax, "n_masked": cnt}, 3
        table = torch.from_numpy(np.ascontiguousarray(video.rainbow_table() if colormap is None else colormap, dtype=np.uint8)).to(dev)
    out_dev = torch.empty(int(offs[-1]) * C, dtype=torch.uint8, device=dev)
    for i, (H, W) in enumerate(sizes):
        o, db = out_dev[int(offs[i]) * C: int(offs[i + 1]) * C], db_all[int(offs[i]): int(offs[i + 1])]
        if depth == "max":
            video.depth8_max(db, H, W, dmax, flipy, rot, out=o)
        else:
            video.depth8_map(db, H, W, dmin, dmax, table, flipy, rot, out=o)
    flat = out_dev.cpu().numpy()
    if same and n:
        depth8 = flat.reshape((n,) + out_sizes[0] + (C,))
    else:
        depth8 = [flat[int(offs[i]) * C: int(offs[i + 1]) * C].reshape(out_sizes[i] + (C,)) for i in range(n)]
    return rgb8, depth8, info


class _FrameLoop:
    """The view loop render_viewpoints and render_video share: views take the streams and work-list slots in turn (frames_in_flight),
    a process group of more than one rank goes through dist.FramePipeline, where view i is completed on the stream of view i + 1.
    run() hands every completed packed frame to `finish(i, packed, stream, slot)` on the stream that completed it; join() puts the
    model back on work list 0 and makes the caller's stream wait for the views' streams."""

    def __init__(self, model, n_views, group, frames_in_flight, deal, deal_group):
        self.model, self.group, self.n = model, group, n_views
        dev = self.dev = model.device
        self.pipe = None
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size(group) > 1:
            from .dist import FramePipeline
            self.pipe = FramePipeline(model, group=group, deal=deal or "bands", deal_group=deal_group)
        if frames_in_flight is None:
            frames_in_flight = int(getattr(model, "frames_in_flight", 2))
        self.copy_stream = torch.cuda.Stream(dev)
        self.caller = torch.cuda.current_stream(dev)
        self.pair = None
        if (frames_in_flight >= 2 and hasattr(model, "use_workspace_slot") and n_views > 1
                and model.use_workspace_slot(0) is not False):      # (False: a model outside the fused shapes, composed forward, one stream)
            self.pair = [torch.cuda.Stream(dev) for _ in range(min(int(frames_in_flight), n_views))]
        self.n_slots = len(self.pair) if self.pair is not None else 2

    def run(self, render_poses, HW, Ks, render_kwargs, flip_x, flip_y, finish):
        model, pipe, pair, caller, n, n_slots = self.model, self.pipe, self.pair, self.caller, self.n, self.n_slots
        n_done = 0                    # (process group: views completed so far; view i - 1 is completed on the stream of view i)
        for i in range(n + (1 if pipe is not None else 0)):
            stream, k = caller, i % n_slots
            if pair is not None:
                stream = pair[k]
                if i < n:
                    model.use_workspace_slot(k)
                if i < n_slots:
                    stream.wait_stream(caller)        # (whatever prepared the model -- bricks, weight images -- ran on the caller's stream)
            with torch.cuda.stream(stream):
                if i == n:
                    packed = pipe.flush()
                elif pipe is None:
                    packed = _render_packed(model, int(HW[i][0]), int(HW[i][1]), Ks[i], render_poses[i], render_kwargs, flip_x, flip_y, self.group)
                else:
                    packed = pipe.submit(int(HW[i][0]), int(HW[i][1]), Ks[i], render_poses[i], **_frame_kwargs(render_kwargs, flip_x, flip_y))
                if packed is not None:
                    finish(n_done, packed.reshape(-1), stream, k)
                    n_done += 1

    def join(self):
        if self.pair is not None:
            self.model.use_workspace_slot(0)
            for st in self.pair:
                self.caller.wait_stream(st)


def _frame_kwargs(render_kwargs, flip_x, flip_y):
    """what a renderer's frame entry takes of the reference's render_kwargs (dist.FramePipeline picks near / far / bg for the bounded family)"""
    kw = {k: render_kwargs[k] for k in ("near", "far", "stepsize", "bg") if k in render_kwargs}
    kw.update(inverse_y=bool(render_kwargs.get("inverse_y", False)), flip_x=flip_x, flip_y=flip_y)
    return kw


def _render_packed(model, H, W, K, c2w, render_kwargs, flip_x, flip_y, group):
    """one view on the current stream -> flat [H*W*5] = rgb(3), depth, alphainv_last per pixel"""
    if FUSED_ASSEMBLY:      # per-ray arrays in ray order -> the frame, one launch (reached with one rank only: no exchange)
        from .dist import FramePipeline
        return FramePipeline(model).render_local(H, W, K, c2w, **_frame_kwargs(render_kwargs, flip_x, flip_y)).reshape(-1)
    if hasattr(model, "fused_supported"):          # bounded / contracted VoxGO renderers: dict of per-ray outputs
        kw = {k: render_kwargs[k] for k in ("near", "far", "stepsize", "bg") if k in render_kwargs}
        out = model.render_view(H, W, K, c2w, inverse_y=bool(render_kwargs.get("inverse_y", False)),
                                flip_x=flip_x, flip_y=flip_y, render_depth=True, **kw)
        rgb, depth, bg = out["rgb_marched"], out["depth"], out["alphainv_last"]
    else:
        rgb, depth, bg = model.render_view(H, W, K, c2w, render_kwargs["stepsize"],
                                           inverse_y=bool(render_kwargs.get("inverse_y", False)),
                                           flip_x=flip_x, flip_y=flip_y, group=group)
    return torch.cat([rgb.reshape(-1, 3), depth.reshape(-1, 1), bg.reshape(-1, 1)], dim=1).reshape(-1)


def _stack(frames, gt_imgs, render_factor, n):
    rgbs = np.array([f[..., 0:3] for f in frames])
    depths = np.array([f[..., 3:4] for f in frames])
    bgmaps = np.array([f[..., 4:5] for f in frames])
    if gt_imgs is None:
        return rgbs, depths, bgmaps
    psnrs = []
    for i in range(n):
        gt = np.asarray(gt_imgs[i])
        if render_factor != 0:
            raise ValueError("ground-truth comparison needs render_factor == 0 (run_render.py:74 compares full frames)")
        psnrs.append(-10.0 * np.log10(np.mean(np.square(rgbs[i] - gt))))          # run_render.py:75
    return rgbs, depths, bgmaps, psnrs
