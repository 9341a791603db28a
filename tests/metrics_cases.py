"""Image pairs of the frame-metric tests (unboundednerfpytorch_amd.metrics, csrc/ugrid_metrics.hip), generated from seeds, and
an independent numpy fp64 statement of the reference's utils.rgb_ssim formula (sliding windows, no scipy).

tests/golden/gen_golden_metrics.py runs the reference's own function on these pairs and stores its maps in
tests/golden/ssim_maps.npz; the GPU tests read that file and this module only."""
import numpy as np

TILE_Y, TILE_X = 32, 54      # map elements per workgroup of k_frame_metrics, per axis (rows, columns)


def _noise_pair(seed, H, W, amp=0.1):
    rs = np.random.RandomState(seed)
    a = rs.rand(H, W, 3).astype(np.float32)
    b = np.clip(a + amp * rs.randn(H, W, 3), 0.0, 1.0).astype(np.float32)
    return a, b


def _flat_bright(seed, H, W):
    """0.9 +- 1e-3: E[x^2] - mu^2 cancels to ~1e-6 against c2 = 9e-4; an fp32 evaluation of the map is off by up to 5.7e-4 here"""
    rs = np.random.RandomState(seed)
    a = (0.9 + 1e-3 * (2.0 * rs.rand(H, W, 3) - 1.0)).astype(np.float32)
    b = (0.9 + 1e-3 * (2.0 * rs.rand(H, W, 3) - 1.0)).astype(np.float32)
    return a, b


def _identical(seed, H, W):
    a = np.random.RandomState(seed).rand(H, W, 3).astype(np.float32)
    return a, a.copy()


def _negated(seed, H, W):
    a = np.random.RandomState(seed).rand(H, W, 3).astype(np.float32)
    return a, (np.float32(1.0) - a).astype(np.float32)


def _constant(seed, H, W):
    """two constant images: the blurred second moment minus the squared mean is zero or a few ulps either side of it (the clamps)"""
    return np.full((H, W, 3), 0.3, np.float32), np.full((H, W, 3), 0.7, np.float32)


_T = (TILE_Y, TILE_X)
# name -> (maker, seed, H, W); frame = map extent + 10.  The four tile-edge shapes put T-1, T, T+1 and 2T+3 on each axis.
PAIRS = {
    "smallest": (_noise_pair, 11, 11, 11),                                      # a 1 x 1 map
    "thin_ragged": (_noise_pair, 12, 13, 75),                                   # 3 map rows, a ragged second axis (65 = 54 + 11)
    "tile_m1_2p3": (_noise_pair, 13, _T[0] - 1 + 10, 2 * _T[1] + 3 + 10),       # map 31 x 111
    "tile_2p3_m1": (_noise_pair, 14, 2 * _T[0] + 3 + 10, _T[1] - 1 + 10),       # map 67 x 53
    "tile_eq_p1": (_noise_pair, 15, _T[0] + 10, _T[1] + 1 + 10),                # map 32 x 55
    "tile_p1_eq": (_noise_pair, 16, _T[0] + 1 + 10, _T[1] + 10),                # map 33 x 54
    "noise": (_noise_pair, 17, 45, 38),                                         # the general path
    "flat_bright": (_flat_bright, 18, 45, 70),                                  # the cancellation case
    "identical": (_identical, 19, 43, 65),                                      # map exactly 1, squared error exactly 0
    "negated": (_negated, 20, 30, 40),                                          # negative covariance: the sign path
    "constant": (_constant, 21, 20, 25),                                        # zero / slightly negative variance: the clamps
}


def pair(name):
    """(img, gt) float32 [H,W,3] of the named pair"""
    maker, seed, H, W = PAIRS[name]
    return maker(seed, H, W)


def gaussian_taps(filter_size=11, filter_sigma=1.5):
    x = (np.arange(filter_size, dtype=np.float64) - filter_size // 2) / filter_sigma
    f = np.exp(-0.5 * x * x)
    return f / f.sum()


def ssim_map_numpy(img0, img1, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """the SSIM map [(H-f+1),(W-f+1),3] in fp64 of two float32 images: the products of the inputs in float32 (as numpy forms them
    on float32 arrays), everything behind them in float64"""
    img0 = np.asarray(img0, dtype=np.float32)
    img1 = np.asarray(img1, dtype=np.float32)
    f = gaussian_taps(filter_size, filter_sigma)
    win = np.lib.stride_tricks.sliding_window_view

    def conv(z, axis):
        # out[i] = sum_k f[k] z[i + f-1 - k], the taps added one after the other in the order of a convolution sum: on the nearly
        # flat pair the order of these 11 additions alone moves the map by 1.4e-12 (a matrix product of the windows with the taps
        # adds them differently), so the bound of 1e-12 against the reference needs the order a direct convolution uses
        w = win(z, filter_size, axis=axis)
        acc = np.zeros(w.shape[:-1], dtype=np.float64)
        for k in range(filter_size):
            acc = acc + f[k] * w[..., filter_size - 1 - k]
        return acc

    def blur(z):
        return conv(conv(z.astype(np.float64), 0), 1)      # rows' axis first, like the reference

    mu0, mu1 = blur(img0), blur(img1)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    s00 = np.maximum(0.0, blur(img0 * img0) - mu00)
    s11 = np.maximum(0.0, blur(img1 * img1) - mu11)
    s01 = blur(img0 * img1) - mu01
    s01 = np.sign(s01) * np.minimum(np.sqrt(s00 * s11), np.abs(s01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    return ((2.0 * mu01 + c1) * (2.0 * s01 + c2)) / ((mu00 + mu11 + c1) * (s00 + s11 + c2))


def sq_err_sum_numpy(img, gt):
    """numpy's fp64 sum of the float32 squares of the float32 differences"""
    d = np.asarray(img, dtype=np.float32) - np.asarray(gt, dtype=np.float32)
    return float(np.sum(np.square(d), dtype=np.float64))
