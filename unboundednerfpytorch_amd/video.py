"""8-bit video frames on the device: the bytes the reference's render program (FourierGrid/run_render.py) forms on the host
with numpy from render_viewpoints' float stacks, made from the packed frame [H*W,5] where it lies (csrc/ugrid_video.hip):

    frame_rgb8(packed, H, W, flipy, k)        utils.to8b(rgbs) behind render_video_flipy / render_video_rot90      (:93-103, :261/:283/:307)
    depth8_max(db, H, W, dmax, flipy, k)      utils.to8b(1 - depths / np.max(depths))                              (:284)
    depthvis_select(db, ranks, thres)         the order statistics of depths_vis[bgmaps < thres]                   (:308-313)
    depth8_map(db, H, W, dmin, dmax, table)   to8b(cmap(1 - clip((depths_vis - dmin) / (dmax - dmin), 0, 1)))      (:314-315)

and two host functions: rainbow_table() (matplotlib's `rainbow` as the 256 x 3 bytes to8b makes of it, matplotlib not needed) and
percentile_from_order_stats() (numpy's `linear` percentile from a handful of order statistics).  Every op runs on the current
stream; only depthvis_select reads anything back.  run_render.render_video drives them."""
import ctypes

import numpy as np
import torch

from . import _lib

MAX_RANKS = 4


def orientation(H, W, flipy=False, k=0):
    """(H', W', s0, si, sj): np.rot90(np.flip(img, 0) if flipy else img, k, axes=(0,1)) of an H x W image puts source pixel
    s0 + i*si + j*sj (row-major index) at output pixel (i, j) of the H' x W' result.  Host arithmetic of the library."""
    plan = (ctypes.c_int64 * 5)()
    _lib.check(_lib.load().ugrid_video_plan(int(H), int(W), int(bool(flipy)), int(k), ctypes.cast(plan, ctypes.c_void_p)), "ugrid_video_plan")
    return tuple(int(v) for v in plan)


def out_shape(H, W, k=0):
    return (int(W), int(H)) if int(k) % 2 else (int(H), int(W))


def _check_out(out, n_bytes, dev):
    if out is None:
        return torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    if not (out.is_cuda and out.device == dev and out.dtype == torch.uint8 and out.numel() == n_bytes and out.is_contiguous()):
        raise RuntimeError("out: %d contiguous uint8 elements on %s expected" % (n_bytes, dev))
    return out


def _check_db(db, H, W):
    if not isinstance(db, torch.Tensor) or not db.is_cuda:
        raise RuntimeError("db must be a CUDA tensor")
    _lib.require_f32(("db", db))
    if not db.is_contiguous() or db.numel() != 2 * H * W:
        raise RuntimeError("db: [%d,2] contiguous expected (got %s)" % (H * W, tuple(db.shape)))


def depth_key_to_float(key):
    """the float behind the order-preserving uint32 key frame_rgb8 keeps in its `dmax` word"""
    key = int(key) & 0xFFFFFFFF
    u = (key & 0x7FFFFFFF) if key & 0x80000000 else (~key & 0xFFFFFFFF)
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def frame_rgb8(packed, H, W, flipy=False, k=0, out=None, db=None, dmax=None):
    """packed: float32 device rows [H*W, >= 5] (unit stride inside a row): what FramePipeline.render_local / submit return.  Returns
    uint8 [H',W',3] = to8b(rgb) in the orientation np.rot90(np.flip(img, 0) if flipy else img, k).  NaN gives 0.
    out: uint8 device tensor of H*W*3 contiguous elements (any alignment: a slice of a byte buffer qualifies).
    db: float32 [H*W,2] to receive (depth, alphainv_last) per pixel in source order.  dmax: an int32 device tensor of one element,
    zero before the first call, that keeps the maximum depth of every frame handed it (decode with depth_key_to_float)."""
    H, W = int(H), int(W)
    if not isinstance(packed, torch.Tensor) or not packed.is_cuda:
        raise RuntimeError("packed must be a CUDA tensor")
    _lib.require_f32(("packed", packed))
    if packed.dim() != 2 or packed.shape[0] != H * W or packed.shape[1] < 5 or packed.stride(1) != 1 or packed.stride(0) < packed.shape[1]:
        raise ValueError("packed: [%d,>=5] rows expected for a %d x %d frame (got %s)" % (H * W, H, W, tuple(packed.shape)))
    dev = packed.device
    Ho, Wo = out_shape(H, W, k)
    out = _check_out(out, H * W * 3, dev)
    if db is not None:
        _check_db(db, H, W)
    if dmax is not None and not (dmax.is_cuda and dmax.dtype == torch.int32 and dmax.numel() == 1):
        raise RuntimeError("dmax: one int32 element on the device expected")
    with _lib.guard(dev):
        _lib.check(_lib.load().ugrid_frame_rgb8(packed.data_ptr(), int(packed.stride(0)), H, W, int(bool(flipy)), int(k), out.data_ptr(),
                                                _lib.ptr(db), _lib.ptr(dmax), _lib.stream_of(packed)), "ugrid_frame_rgb8")
    return out.view(Ho, Wo, 3)


def depth8_max(db, H, W, dmax, flipy=False, k=0, out=None):
    """uint8 [H',W',1] = to8b(1 - d / dmax) in fp32 from db [H*W,2]; dmax (a host float) == 0 gives zeros"""
    H, W = int(H), int(W)
    _check_db(db, H, W)
    Ho, Wo = out_shape(H, W, k)
    out = _check_out(out, H * W, db.device)
    with _lib.guard(db.device):
        _lib.check(_lib.load().ugrid_depth8_max(db.data_ptr(), H, W, int(bool(flipy)), int(k), float(dmax), out.data_ptr(),
                                                _lib.stream_of(db)), "ugrid_depth8_max")
    return out.view(Ho, Wo, 1)


def depth8_map(db, H, W, dmin, dmax, table, flipy=False, k=0, out=None):
    """uint8 [H',W',3] = table[(int)((1 - clip((v - dmin) / (dmax - dmin), 0, 1)) * 256)] in fp64 with v = d*(1 - b) + b in fp32;
    table: uint8 device tensor [256,3] (rainbow_table() uploaded); NaN gives (0,0,0)"""
    H, W = int(H), int(W)
    _check_db(db, H, W)
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.device == db.device and table.dtype == torch.uint8
            and tuple(table.shape) == (256, 3) and table.is_contiguous()):
        raise RuntimeError("table: a contiguous uint8 [256,3] tensor on %s expected" % (db.device,))
    Ho, Wo = out_shape(H, W, k)
    out = _check_out(out, H * W * 3, db.device)
    with _lib.guard(db.device):
        _lib.check(_lib.load().ugrid_depth8_map(db.data_ptr(), H, W, int(bool(flipy)), int(k), float(dmin), float(dmax), table.data_ptr(),
                                                out.data_ptr(), _lib.stream_of(db)), "ugrid_depth8_map")
    return out.view(Ho, Wo, 3)


def depthvis_select(db, ranks=(), thres=0.1, ws=None):
    """db: float32 device [n,2] of (depth, alphainv_last), any number of frames.  Returns (cnt, values): cnt = pixels with
    b < float32(thres); values = float32 array, values[r] = the ranks[r]-th smallest (0-based) v = d*(1 - b) + b among them --
    exact, the same in every run (radix select, no sort).  ranks: at most 4, ascending, each < cnt: ValueError otherwise (a rank
    beyond the count is reported once the count is known; nothing is returned then).  Synchronises the current stream."""
    if not isinstance(db, torch.Tensor) or not db.is_cuda:
        raise RuntimeError("db must be a CUDA tensor")
    _lib.require_f32(("db", db))
    if not db.is_contiguous() or db.numel() % 2:
        raise RuntimeError("db: [n,2] contiguous expected (got %s)" % (tuple(db.shape),))
    ranks = [int(r) for r in ranks]
    m = len(ranks)
    if m > MAX_RANKS:
        raise ValueError("%d ranks: at most %d per call" % (m, MAX_RANKS))
    if any(r < 0 for r in ranks) or any(b < a for a, b in zip(ranks, ranks[1:])):
        raise ValueError("ranks %s: ascending non-negative ranks expected" % (ranks,))
    lib = _lib.load()
    n = db.numel() // 2
    need = int(lib.ugrid_depthvis_select_ws_bytes())
    c_ranks = (ctypes.c_int64 * max(m, 1))(*ranks)
    c_vals = (ctypes.c_float * max(m, 1))()
    c_cnt = ctypes.c_int64(-1)
    with _lib.guard(db.device):
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=db.device)
        elif not ws.is_cuda or ws.device != db.device or ws.numel() * ws.element_size() < need or not ws.is_contiguous():
            raise RuntimeError("ws: %d contiguous bytes on %s expected" % (need, db.device))
        err = lib.ugrid_depthvis_select(db.data_ptr() if n else None, n, float(thres), m, ctypes.cast(c_ranks, ctypes.c_void_p),
                                        ctypes.addressof(c_cnt), ctypes.cast(c_vals, ctypes.c_void_p), ws.data_ptr(), _lib.stream_of(db))
    if err == 1 and m and (c_cnt.value >= 0 or n == 0):
        raise ValueError("ranks %s: %d pixels take part" % (ranks, max(c_cnt.value, 0)))
    _lib.check(err, "ugrid_depthvis_select")
    return int(c_cnt.value), np.array(c_vals[:m], dtype=np.float32)


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)      # FourierGrid/utils.py


def rainbow_table():
    """uint8 [256,3]: to8b of matplotlib's `rainbow` lookup table, from its published definition (matplotlib/_cm.py, _rainbow_data:
    red |2x - 0.5|, green sin(pi x), blue cos(pi x / 2) on linspace(0, 1, 256), clipped to [0,1] in float64) -- entry i is what
    to8b(plt.get_cmap('rainbow')(x)[..., :3]) gives for every x with (int)(x*256) == i.  matplotlib is not imported."""
    x = np.linspace(0.0, 1.0, 256)
    lut = np.stack([np.abs(2 * x - 0.5), np.sin(x * np.pi), np.cos(x * np.pi / 2)], axis=1)
    return to8b(np.clip(np.array(lut, dtype=float), 0, 1))


def percentile_from_order_stats(cnt, q, select):
    """np.percentile(values, q) (method 'linear') of `cnt` float32 values known only through their order statistics:
    select(ranks) -> the values of the given ascending 0-based ranks (at most 4 per call; depthvis_select's second result).
    q: a sequence (or array) of percentiles, as the reference passes q=[5, 95]; a scalar counts as a sequence of one.  Follows
    numpy's own steps -- quantile q / float32(100), virtual index (cnt - 1) * quantile in float64, neighbours floor and floor + 1
    (both the last element at or beyond it), weight = virtual index - floor, _lerp with its branch for a weight >= 0.5 -- and
    returns the float64 array np.percentile returns for that q.  (A NaN among the values is not looked for.)"""
    cnt = int(cnt)
    if cnt < 1:
        raise ValueError("percentile of no values")
    q = np.atleast_1d(np.asanyarray(q))
    if q.ndim != 1 or not np.all((q >= 0) & (q <= 100)):
        raise ValueError("Percentiles must be in the range [0, 100]")
    quantiles = np.true_divide(q, np.float32(100))
    vi = np.asanyarray((cnt - 1) * quantiles)
    prev = np.asanyarray(np.floor(vi))
    nxt = np.asanyarray(prev + 1)
    above = vi >= cnt - 1
    prev[above] = -1
    nxt[above] = -1
    prev, nxt = prev.astype(np.intp), nxt.astype(np.intp)
    gamma = np.asanyarray(vi - prev, dtype=vi.dtype)
    want = sorted(set((prev % cnt).tolist()) | set((nxt % cnt).tolist()))
    got = {}
    for s in range(0, len(want), MAX_RANKS):
        part = want[s:s + MAX_RANKS]
        for r, v in zip(part, select(part)):
            got[r] = np.float32(v)
    a = np.array([got[r] for r in (prev % cnt).tolist()], dtype=np.float32)
    b = np.array([got[r] for r in (nxt % cnt).tolist()], dtype=np.float32)
    diff_b_a = np.subtract(b, a)
    lerp = np.asanyarray(np.add(a, diff_b_a * gamma))
    np.subtract(b, diff_b_a * (1 - gamma), out=lerp, where=gamma >= 0.5, casting='unsafe', dtype=type(lerp.dtype))
    return lerp


__all__ = ["orientation", "out_shape", "frame_rgb8", "depth8_max", "depth8_map", "depthvis_select", "depth_key_to_float", "to8b",
           "rainbow_table", "percentile_from_order_stats", "MAX_RANKS"]
