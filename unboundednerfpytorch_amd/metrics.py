"""Image metrics on the device: the squared error behind PSNR and the SSIM of the reference's `utils.rgb_ssim`
(FourierGrid/utils.py:79-125), which every evaluation command of the reference asks for with --eval_ssim and which costs
seconds per 1080p frame in its scipy form.  One HIP kernel (csrc/ugrid_metrics.hip, C entry point ugrid_frame_metrics) reads a
rendered frame where it lies on the device and leaves two fp64 sums there; nothing in this module reads them back except
rgb_ssim(), whose contract is to return a Python float.

    sums = frame_metrics(img, gt)                  # device [2] float64: sum (img - gt)^2, sum of the SSIM map
    psnr_from_sums(sums, H, W), ssim_from_sums(sums, H, W)
    rgb_ssim(img0, img1, max_val)                  # the reference's function, same positional signature

Arithmetic: that of rgb_ssim on float32 images -- the products of the inputs in fp32, both blur passes and the pointwise
formula in fp64 -- so the map agrees with the reference's to summation order (1e-11), not to an fp32 evaluation's 5.7e-4."""
import numpy as np
import torch

from . import _lib

TILE_Y, TILE_X = 32, 54          # map elements per workgroup (csrc/ugrid_metrics.hip); ws_bytes = 16 per tile


def workspace_bytes(H, W):
    """bytes of the scratch ugrid_frame_metrics needs for an H x W frame (one pair of doubles per tile of the map)"""
    return int(_lib.load().ugrid_frame_metrics_ws_bytes(int(H), int(W)))


def _pixels(name, t, H, W):
    """(tensor, H, W, pixel stride in floats) of an image argument: [H,W,3] contiguous, or [H*W,k] rows (k >= 3, unit stride
    inside a row -- a column slice of a wider row-major tensor qualifies: the kernel reads the first three floats of every row)"""
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s: a torch tensor expected (got %s); rgb_ssim() takes numpy arrays" % (name, type(t).__name__))
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA tensor" % name)
    _lib.require_f32((name, t))
    if t.dim() == 3:
        if t.shape[2] != 3:
            raise ValueError("%s: [H,W,3] expected (got %s)" % (name, tuple(t.shape)))
        if not t.is_contiguous():
            raise RuntimeError("%s must be contiguous" % name)
        if (H is not None and H != t.shape[0]) or (W is not None and W != t.shape[1]):
            raise ValueError("%s is %s but H, W = %s, %s" % (name, tuple(t.shape), H, W))
        return t, int(t.shape[0]), int(t.shape[1]), 3
    if t.dim() == 2:
        if H is None or W is None:
            raise ValueError("%s: [H*W,k] rows need H and W" % name)
        if t.shape[0] != H * W or t.shape[1] < 3:
            raise ValueError("%s: [%d,>=3] rows expected for a %d x %d frame (got %s)" % (name, H * W, H, W, tuple(t.shape)))
        if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
            raise RuntimeError("%s must be contiguous within its rows" % name)
        return t, int(H), int(W), int(t.stride(0))
    raise ValueError("%s: [H,W,3] or [H*W,k] expected (got %s)" % (name, tuple(t.shape)))


def frame_metrics(img, gt, max_val=1.0, return_map=False, out=None, H=None, W=None, ws=None,
                  filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """img, gt: float32 device tensors, each [H,W,3] or [H*W,k] rows with H and W given (the frame loop's packed [H*W,5] result is
    read in place, with stride 5).  Returns `sums`, a float64 device tensor [2]: sums[0] = sum over all H*W*3 elements of
    (img - gt)^2 (difference and square in fp32 as numpy forms them on float32 arrays, the sum in fp64), sums[1] = sum over the
    [(H-10),(W-10),3] SSIM map; with return_map=True, (sums, map) with the map as float64 [(H-10),(W-10),3].  Everything is enqueued
    on the current stream and nothing is read back.  out: a float64 device tensor of two contiguous elements to write the sums to
    (e.g. a row of a caller's [N,2] tensor) -- returned in place of a new one.  ws: scratch of at least workspace_bytes(H, W)
    bytes (any dtype; default: allocated per call).  Deterministic: the same inputs give the same bits.
    RuntimeError for host tensors, ValueError for frames smaller than 11 in either axis or of different shapes."""
    img, H0, W0, s0 = _pixels("img", img, H, W)
    gt, H1, W1, s1 = _pixels("gt", gt, H, W)
    if (H0, W0) != (H1, W1):
        raise ValueError("img is %d x %d, gt is %d x %d" % (H0, W0, H1, W1))
    if gt.device != img.device:
        raise RuntimeError("img is on %s, gt on %s" % (img.device, gt.device))
    if H0 < 11 or W0 < 11:
        raise ValueError("frame %d x %d: the 11-tap SSIM window needs at least 11 x 11 pixels" % (H0, W0))
    if filter_size != 11:
        raise ValueError("filter_size %s: the kernel is built for the reference's default, 11" % (filter_size,))
    lib = _lib.load()
    need = int(lib.ugrid_frame_metrics_ws_bytes(H0, W0))
    with _lib.guard(img.device):
        if out is None:
            out = torch.empty(2, dtype=torch.float64, device=img.device)
        elif not (out.is_cuda and out.device == img.device and out.dtype == torch.float64 and out.numel() == 2 and out.is_contiguous()):
            raise RuntimeError("out: two contiguous float64 elements on %s expected" % (img.device,))
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=img.device)
        elif not ws.is_cuda or ws.device != img.device or ws.numel() * ws.element_size() < need or not ws.is_contiguous():
            raise RuntimeError("ws: %d contiguous bytes on %s expected" % (need, img.device))
        ssim_map = torch.empty((H0 - 10, W0 - 10, 3), dtype=torch.float64, device=img.device) if return_map else None
        _lib.check(lib.ugrid_frame_metrics(img.data_ptr(), s0, gt.data_ptr(), s1, H0, W0, int(filter_size), float(filter_sigma),
                                           float(k1), float(k2), float(max_val), out.data_ptr(), _lib.ptr(ssim_map), ws.data_ptr(),
                                           _lib.stream_of(img)), "ugrid_frame_metrics")
    return (out, ssim_map) if return_map else out


def psnr_from_sums(sums, H, W, max_val=1.0):
    """PSNR = 10 log10(max_val^2 / mse) from sums[..., 0] of frame_metrics for H x W frames: a tensor in, a tensor out (no host
    read); a float / numpy array in, the same out.  (max_val = 1: -10 log10(mse), the reference's run_render.py:75.)"""
    n = float(H) * float(W) * 3.0
    if isinstance(sums, torch.Tensor):
        return 10.0 * torch.log10(float(max_val) ** 2 * n / sums[..., 0])
    s = np.asarray(sums, dtype=np.float64)[..., 0]
    return 10.0 * np.log10(float(max_val) ** 2 * n / s)


def ssim_from_sums(sums, H, W):
    """mean of the SSIM map from sums[..., 1] of frame_metrics for H x W frames (tensor in, tensor out; numpy likewise)"""
    n = float(H - 10) * float(W - 10) * 3.0
    if isinstance(sums, torch.Tensor):
        return sums[..., 1] / n
    return np.asarray(sums, dtype=np.float64)[..., 1] / n


def _to_device_f32(a, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32)).to(device)


def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """The reference's utils.rgb_ssim (same positional signature) on the GPU.  img0, img1: [H,W,3] numpy arrays or tensors, on the
    host or the device; host input is converted to float32 and uploaded to the current device (device tensors are used where they
    are).  float64 input is ROUNDED to float32 first: the reference's loaders hand float32 images over (and its renderer float32
    frames), for which the result equals the reference's to summation order; on genuinely float64 images the reference would blur
    the unrounded values.  Returns the mean SSIM as a Python float, or with return_map=True the [(H-10),(W-10),3] map as a float64
    numpy array -- both read back from the device, as the signature demands.  Only filter_size == 11 is built."""
    shp0, shp1 = tuple(img0.shape), tuple(img1.shape)
    if len(shp0) != 3 or shp0[-1] != 3 or shp0 != shp1:            # (the reference asserts the same three things)
        raise ValueError("rgb_ssim: two [H,W,3] images of one shape expected (got %s and %s)" % (shp0, shp1))
    dev = None
    for a in (img0, img1):
        if isinstance(a, torch.Tensor) and a.is_cuda:
            dev = a.device
            break
    if dev is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    a, b = _to_device_f32(img0, dev), _to_device_f32(img1, dev)
    res = frame_metrics(a, b, max_val=max_val, return_map=return_map, filter_size=filter_size, filter_sigma=filter_sigma, k1=k1, k2=k2)
    if return_map:
        return res[1].cpu().numpy()
    return mean_ssim(float(res[1].item()), shp0[0], shp0[1])


def mean_ssim(map_sum, H, W):
    """the mean of an H x W frame's SSIM map from its sum on the host (rgb_ssim and the frame loop divide the same way, so a frame
    scored by either gets the same float)"""
    return float(map_sum) / (float(H - 10) * float(W - 10) * 3.0)


__all__ = ["frame_metrics", "rgb_ssim", "psnr_from_sums", "ssim_from_sums", "mean_ssim", "workspace_bytes", "TILE_Y", "TILE_X"]
