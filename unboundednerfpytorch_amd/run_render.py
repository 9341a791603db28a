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
renders.  In a single process the same kernel puts the frame together from the per-ray arrays (FUSED_ASSEMBLY)."""
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
    dev = model.device
    pipe = None
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size(group) > 1:
        from .dist import FramePipeline
        pipe = FramePipeline(model, group=group, deal=deal or "bands", deal_group=deal_group)
    if frames_in_flight is None:
        frames_in_flight = int(getattr(model, "frames_in_flight", 2))
    copy_stream = torch.cuda.Stream(dev)
    caller = torch.cuda.current_stream(dev)
    pair = None
    if (frames_in_flight >= 2 and hasattr(model, "use_workspace_slot") and len(render_poses) > 1
            and model.use_workspace_slot(0) is not False):      # (False: a model outside the fused shapes, composed forward, one stream)
        pair = [torch.cuda.Stream(dev) for _ in range(min(int(frames_in_flight), len(render_poses)))]
    n = len(render_poses)
    n_slots = len(pair) if pair is not None else 2
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
                packed = _render_packed(model, int(HW[i][0]), int(HW[i][1]), Ks[i], render_poses[i], render_kwargs, flip_x, flip_y, group)
            else:
                packed = pipe.submit(int(HW[i][0]), int(HW[i][1]), Ks[i], render_poses[i], **_frame_kwargs(render_kwargs, flip_x, flip_y))
            if packed is not None:
                finish(n_done, packed.reshape(-1), stream, k)
                n_done += 1
    while pending:
        drain(*pending.pop(0))
    if pair is not None:
        model.use_workspace_slot(0)
        for st in pair:
            caller.wait_stream(st)
    res = _stack(frames, gt_imgs, render_factor, n)
    if not eval_ssim:
        return res
    host_sums = sums.cpu().numpy()        # the one read of the metric (the caller's stream has joined every view's stream above)
    ssims = [metrics.mean_ssim(host_sums[i, 1], int(HW[i][0]), int(HW[i][1])) for i in range(n)]
    return res + (ssims,)


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
