"""The numpy reference of the video ops (unboundednerfpytorch_amd/video.py, csrc/ugrid_video.hip) and the builders of their test
cases.  The reference is the literal lines of the reference's render program (FourierGrid/run_render.py, utils.py) applied to the
float stacks render_viewpoints returns; the only substitution is the colour map, a 256-entry table looked up the way
matplotlib.colors.Colormap.__call__ looks floats up (x*N truncated, N -> N-1, NaN -> the all-zero "bad" colour)."""
import numpy as np

to8b = lambda x: (255*np.clip(x,0,1)).astype(np.uint8)      # utils.py


def orient(frames, flipy, k):
    """run_render.py:93-103 on a list of [H,W,C] frames"""
    frames = list(frames)
    if flipy:
        for i in range(len(frames)):
            frames[i] = np.flip(frames[i], axis=0)
    if k != 0:
        for i in range(len(frames)):
            frames[i] = np.rot90(frames[i], k=k, axes=(0,1))
    return frames


def ref_to8b(x):
    """to8b with this library's rule for NaN (numpy's cast of NaN is undefined): 0"""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), np.uint8(0), to8b(np.where(np.isnan(x), 0, x)))


def ref_rgb8(rgbs, flipy=False, k=0):
    """:261 / :283 / :307  utils.to8b(rgbs), frame by frame"""
    return [ref_to8b(f) for f in orient(rgbs, flipy, k)]


def ref_depth8_max(depths, flipy=False, k=0, dmax=None):
    """:284  utils.to8b(1 - depths / np.max(depths)); np.max over ALL frames; a zero maximum gives zeros (stated rule)"""
    frames = orient(depths, flipy, k)
    dmax = np.max([np.max(d) for d in depths]) if dmax is None else np.float32(dmax)
    if dmax == 0:
        return [np.zeros(f.shape, np.uint8) for f in frames], dmax
    with np.errstate(invalid="ignore", divide="ignore"):
        return [ref_to8b(1 - f / dmax) for f in frames], dmax


def masked_values(depths, bgmaps, thres=0.1):
    """depths_vis[bgmaps < thres] over all frames (:308-309, :313)"""
    out = []
    for d, b in zip(depths, bgmaps):
        with np.errstate(invalid="ignore", over="ignore"):
            depths_vis = d * (1-b) + b
        out.append(depths_vis[b < np.float32(thres)])
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def lookup(table, x):
    """to8b(cmap(x)[..., :3]) for a colour map given as its to8b table [256,3]: matplotlib's float lookup"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        xa = x * 256
        bad = np.isnan(xa)
        xa = np.where(bad, 0, xa)
        xa[xa == 256] = 255
        i = np.clip(xa, 0, 255).astype(int)
    out = np.asarray(table)[i]
    out[bad] = 0
    return out


def ref_depth8_map(depths, bgmaps, table, q=(5, 95), thres=0.1, flipy=False, k=0, dmin=None, dmax=None):
    """:308-315; returns (frames or None, dmin, dmax, n_masked).  dmin / dmax given: the percentile step is skipped."""
    depths, bgmaps = orient(depths, flipy, k), orient(bgmaps, flipy, k)
    vals = masked_values(depths, bgmaps, thres)
    if dmin is None:
        if vals.size == 0:
            return None, None, None, 0
        dmin, dmax = np.percentile(vals, q=list(q))
    dmin, dmax = np.float64(dmin), np.float64(dmax)      # (what np.percentile returns: the expression below then runs in float64)
    frames = []
    for d, b in zip(depths, bgmaps):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            depths_vis = d * (1-b) + b
            x = 1 - np.clip((depths_vis - dmin) / (dmax - dmin), 0, 1)
        frames.append(lookup(table, x).squeeze(-2) if x.shape[-1] == 1 else lookup(table, x))
    return frames, dmin, dmax, int(vals.size)


# ------------------------------------------------------------------------------------------------------------------ case builders
SIZES = ((1, 1), (8, 8), (9, 13), (16, 24), (37, 53))          # 9 x 13: 351 output bytes; 37 x 53: several workgroups' worth of chunks
ORIENTATIONS = [(f, k) for f in (False, True) for k in (0, 1, 2, 3)] + [(False, -1), (True, 5)]


def special_values():
    """exact 0, 1, j/255 and the fp32 neighbours of j/255 on both sides, -0.0, +-inf, NaN"""
    j = (np.arange(256) / 255.0).astype(np.float32)
    vals = [j, np.nextafter(j, np.float32(-1)), np.nextafter(j, np.float32(2)),
            (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32),
            np.array([0.0, 1.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45, 0.5], np.float32)]
    return np.concatenate(vals).astype(np.float32)


def packed_frame(seed, H, W, stride=5, depth_hi=40.0):
    """a packed frame [H*W, stride] float32: rgb random in [-0.5, 1.5] with the special values sprinkled in (wherever the frame is
    large enough, each at least once), depth in [0, depth_hi], alphainv_last in [0, 1] with a share exactly 0 / 1; columns beyond
    the fifth hold a sentinel the kernels must not read as data"""
    rs = np.random.RandomState(seed)
    a = np.full((H * W, stride), 7.5, np.float32)
    a[:, 0:3] = rs.uniform(-0.5, 1.5, (H * W, 3)).astype(np.float32)
    sp = special_values()
    flat = a[:, 0:3].reshape(-1).copy()
    n = min(sp.size, flat.size)
    pos = rs.permutation(flat.size)[:n]
    flat[pos] = sp[rs.permutation(sp.size)[:n]] if n < sp.size else sp
    a[:, 0:3] = flat.reshape(-1, 3)
    a[:, 3] = rs.uniform(0.0, depth_hi, H * W).astype(np.float32)
    b = rs.uniform(0.0, 1.0, H * W).astype(np.float32)
    b[rs.uniform(size=H * W) < 0.1] = 0.0
    b[rs.uniform(size=H * W) < 0.1] = 1.0
    a[:, 4] = b
    return a


def split(frame, H, W):
    """(rgb [H,W,3], depth [H,W,1], bgmap [H,W,1]) of a packed frame, as render_viewpoints returns them"""
    f = np.ascontiguousarray(frame[:, :5]).reshape(H, W, 5)
    return f[..., 0:3], f[..., 3:4], f[..., 4:5]


def index_image(H, W):
    return np.arange(H * W, dtype=np.int64).reshape(H, W)


def select_sets():
    """name -> (d, b) float32 arrays whose masked values exercise the radix select: see tests/test_gpu_video.py"""
    rs = np.random.RandomState(11)
    sets = {}
    for cnt in (0, 1, 2, 63, 64, 65, 2049):
        n = cnt + 37
        d = rs.uniform(0.0, 40.0, n).astype(np.float32)
        b = np.full(n, 0.5, np.float32)
        b[rs.permutation(n)[:cnt]] = rs.uniform(0.0, 0.09, cnt).astype(np.float32)
        sets["cnt%d" % cnt] = (d, b)
    n = 100003
    zeros = np.zeros(n, np.float32)
    sets["all_equal"] = (np.full(n, 3.25, np.float32), zeros)
    base = np.float32(1.5).view(np.uint32)
    sets["last10bits"] = ((base + rs.randint(0, 1024, n).astype(np.uint32)).view(np.float32), zeros)      # consecutive floats: pass 3 decides
    sets["spread"] = ((rs.uniform(-1, 1, n) * np.exp2(rs.uniform(-60, 60, n))).astype(np.float32), zeros)  # many top-11-bit bins
    neg = np.concatenate([-rs.uniform(0, 1e-38, n // 3), rs.uniform(-2, 2, n // 3), [0.0, -0.0, 1e-45, -1e-45, 1.17e-38, -1.17e-38]])
    neg = neg.astype(np.float32)
    sets["neg_denormal"] = (neg, np.zeros(neg.size, np.float32))
    d = rs.uniform(0.0, 40.0, n).astype(np.float32)
    b = rs.uniform(0.0, 0.2, n).astype(np.float32)
    t = np.float32(0.1)
    b[:300] = np.tile([t, np.nextafter(t, np.float32(0)), np.nextafter(t, np.float32(1))], 100)     # the threshold and its neighbours
    sets["threshold"] = (d, b)
    return sets


def ranks_for(cnt):
    """ranks 0, cnt - 1, the pair around 5 % and the pair around 95 %, in groups of at most four ascending ranks"""
    if cnt == 0:
        return []
    lo, hi = int(np.floor((cnt - 1) * 0.05)), int(np.floor((cnt - 1) * 0.95))
    pairs = sorted({lo, min(lo + 1, cnt - 1), hi, min(hi + 1, cnt - 1)})
    return [sorted({0, cnt - 1}), pairs]


# ------------------------------------------------------------------------------------------------------------------ end to end
def make_renderer(name, dev):
    """the G = 16 DirectVoxGO / FourierGrid renderer on synthetic parameters (tests/synth.py) and its render_kwargs"""
    if name == "dvgo":
        from test_dvgo import dvgo_state
        from unboundednerfpytorch_amd.dvgo_render import DirectVoxGORenderer
        state, _ = dvgo_state(79, 16, 12, True, 8.0, 9.0, [-0.67, -1.2, -0.37], [0.67, 1.2, 1.03])
        return DirectVoxGORenderer(state, dev), dict(near=2.0, far=6.0, stepsize=0.5, bg=1)
    from test_oracle_golden import make_state
    from unboundednerfpytorch_amd.fourier_render import FourierGridRenderer
    return FourierGridRenderer(make_state(seed=5, G=16, F=3, C=12, pe=4, norm="inf", thres=1e-4, dm=6.0, ds=12.0), dev), dict(stepsize=0.5)


def views(name, sizes=((16, 24),) * 3):
    """render_viewpoints' (poses, HW, Ks) for len(sizes) views with different poses (16 x 24 takes block order, 13 x 7 image order)"""
    poses, HW, Ks = [], [], []
    for i, (H, W) in enumerate(sizes):
        f = 60.0 if name == "dvgo" else 30.0
        Ks.append([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
        if name == "dvgo":
            c2w = [[-0.9999, 0.0042, -0.0133, -0.0538 + 0.03 * i], [-0.0140, -0.2997, 0.9539, 3.8455], [0.0, 0.9540, 0.2997, 1.2081 + 0.01 * i]]
        else:
            c2w = [[1.0, 0, 0, 0.1 + 0.05 * i], [0, 0.8, 0.6, -0.2], [0, -0.6, 0.8, 0.3 + 0.04 * i]]
        poses.append(np.array(c2w, dtype=np.float32))
        HW.append((H, W))
    return poses, HW, Ks
