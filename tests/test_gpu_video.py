"""The video ops on the GPU (csrc/ugrid_video.hip, video.py, run_render.render_video) against the literal numpy lines of the
reference's render program (tests/video_cases.py).  Every comparison is exact: np.array_equal on bytes, no pixel set aside."""
import ctypes
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import video_cases as vc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, PAD = 0xA5, 256


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def _byte_out(n, off=0):
    """(buffer, view): n output bytes `off` bytes beyond a 16-byte boundary, 256 sentinel bytes on both sides"""
    buf = torch.full((PAD + off + n + PAD,), SENT, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[PAD + off: PAD + off + n]


def _sentinels_survive(buf, off, n):
    b = buf.cpu().numpy()
    return bool((b[: PAD + off] == SENT).all() and (b[PAD + off + n:] == SENT).all())


def _db_out(n_pix):
    buf = torch.full((64 + 2 * n_pix + 64,), -123.25, dtype=torch.float32, device="cuda")
    return buf, buf[64: 64 + 2 * n_pix].view(n_pix, 2)


def _db_of(frame):
    return np.ascontiguousarray(frame[:, 3:5])


@functools.lru_cache(maxsize=None)
def _frame(H, W, stride=5, seed=3):
    a = vc.packed_frame(seed + 31 * H + W, H, W, stride)
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------------------------------ ugrid_frame_rgb8
@pytest.mark.parametrize("H,W", vc.SIZES)
@pytest.mark.parametrize("stride", [5, 7])
def test_frame_rgb8_every_orientation(H, W, stride):
    from unboundednerfpytorch_amd import video
    frame = _frame(H, W, stride)
    rgb, _, _ = vc.split(frame, H, W)
    t = _dev(frame)
    for flipy, k in vc.ORIENTATIONS:
        want = vc.ref_rgb8([rgb], flipy, k)[0]
        buf, out = _byte_out(H * W * 3)
        dbuf, db = _db_out(H * W)
        got = video.frame_rgb8(t, H, W, flipy, k, out=out, db=db)
        assert tuple(got.shape) == want.shape, (flipy, k)
        assert np.array_equal(got.cpu().numpy(), want), (flipy, k)
        assert _sentinels_survive(buf, 0, H * W * 3), (flipy, k)
        d = dbuf.cpu().numpy()
        assert (d[:64] == -123.25).all() and (d[-64:] == -123.25).all()
        assert np.array_equal(d[64:-64].view(np.uint32), _db_of(frame).reshape(-1).view(np.uint32)), (flipy, k)      # bit for bit, source order
    if H * W * 3 >= vc.special_values().size:          # (the case really holds the values the rule is about)
        assert np.isnan(rgb).any() and np.isinf(rgb).any() and (rgb == 1).any() and (rgb < 0).any() and (rgb > 1).any()


def test_frame_rgb8_tall_frame_rotated():
    from unboundednerfpytorch_amd import video
    H, W = 64, 4
    frame = _frame(H, W)
    got = video.frame_rgb8(_dev(frame), H, W, False, 1)
    assert tuple(got.shape) == (4, 64, 3) and np.array_equal(got.cpu().numpy(), vc.ref_rgb8([vc.split(frame, H, W)[0]], False, 1)[0])


@pytest.mark.parametrize("off", [1, 2, 3, 8, 13])
def test_frame_rgb8_misaligned_out_keeps_its_neighbours(off):
    from unboundednerfpytorch_amd import video
    for H, W in ((1, 1), (9, 13), (16, 24), (37, 53)):
        frame = _frame(H, W)
        t = _dev(frame)
        for flipy, k in ((False, 0), (True, 1), (False, 2)):
            buf, out = _byte_out(H * W * 3, off)
            assert out.data_ptr() % 16 == off
            got = video.frame_rgb8(t, H, W, flipy, k, out=out)
            assert np.array_equal(got.cpu().numpy(), vc.ref_rgb8([vc.split(frame, H, W)[0]], flipy, k)[0]), (H, W, flipy, k)
            assert _sentinels_survive(buf, off, H * W * 3), (H, W, flipy, k)


def test_frame_rgb8_running_depth_maximum_and_repeatability():
    from unboundednerfpytorch_amd import video
    frames = [vc.packed_frame(100 + i, H, W) for i, (H, W) in enumerate(((16, 24), (37, 53), (9, 13)))]
    frames[1][:, 3] *= np.float32(0.5)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    outs = []
    for f, (H, W) in zip(frames, ((16, 24), (37, 53), (9, 13))):
        outs.append(video.frame_rgb8(_dev(f), H, W, True, 3, dmax=word).cpu().numpy())
    got = video.depth_key_to_float(word.item())
    want = np.max([np.max(f[:, 3]) for f in frames])
    assert got.dtype == np.float32 and got == want and want == frames[0][:, 3].max()      # (the maximum lies in the first frame: it is kept)
    again = [video.frame_rgb8(_dev(f), H, W, True, 3).cpu().numpy() for f, (H, W) in zip(frames, ((16, 24), (37, 53), (9, 13)))]
    assert all(np.array_equal(a, b) for a, b in zip(outs, again))
    # negative depths only: the key order must hold below zero too
    neg = vc.packed_frame(5, 8, 8)
    neg[:, 3] = -1.0 - np.abs(neg[:, 3])
    word.zero_()
    video.frame_rgb8(_dev(neg), 8, 8, dmax=word)
    assert video.depth_key_to_float(word.item()) == neg[:, 3].max()


# ------------------------------------------------------------------------------------------------------------------ ugrid_depth8_max
@pytest.mark.parametrize("H,W", vc.SIZES + ((64, 4),))
def test_depth8_max_every_orientation(H, W):
    from unboundednerfpytorch_amd import video
    frame = _frame(H, W)
    _, depth, _ = vc.split(frame, H, W)
    db = _dev(_db_of(frame))
    orientations = vc.ORIENTATIONS if (H, W) != (64, 4) else [(False, 1)]
    for off, (flipy, k) in enumerate(orientations):
        want, dmax = vc.ref_depth8_max([depth], flipy, k)
        buf, out = _byte_out(H * W, off % 4)
        got = video.depth8_max(db, H, W, float(dmax), flipy, k, out=out)
        assert tuple(got.shape) == want[0].shape and np.array_equal(got.cpu().numpy(), want[0]), (flipy, k)
        assert _sentinels_survive(buf, off % 4, H * W)
    assert np.array_equal(video.depth8_max(db, H, W, 0.0, True, 1).cpu().numpy(), vc.ref_depth8_max([depth], True, 1, dmax=0.0)[0][0])
    assert H * W < 64 or len(np.unique(want[0])) > 16


# ------------------------------------------------------------------------------------------------------------------ ugrid_depthvis_select
SETS = vc.select_sets()


def _same_values(got, want):
    """equal as np.sort orders floats: bit for bit, except that -0.0 and +0.0 are one value"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0))))


@pytest.mark.parametrize("name", sorted(SETS))
def test_depthvis_select_equals_numpy_sort(name):
    from unboundednerfpytorch_amd import video
    d, b = SETS[name]
    s = np.sort(vc.masked_values([d], [b]))
    db = _dev(np.stack([d, b], axis=1))
    cnt, vals = video.depthvis_select(db, ())
    assert cnt == s.size and vals.size == 0
    if name.startswith("cnt"):
        assert cnt == int(name[3:])
    if name == "threshold":                             # float32(0.1) itself is out, its lower neighbour in
        t = np.float32(0.1)
        assert cnt == int((b < t).sum()) and (b == t).sum() >= 100 and (b == np.nextafter(t, np.float32(0))).sum() >= 100
    for ranks in vc.ranks_for(cnt):
        c2, got = video.depthvis_select(db, ranks)
        assert c2 == cnt and _same_values(got, s[ranks]), (name, ranks, got, s[ranks])
        assert _same_values(video.depthvis_select(db, ranks)[1], got)
    if cnt:
        # the percentile the reference takes: numpy's own value
        want = np.percentile(vc.masked_values([d], [b]), q=[5, 95])
        got = video.percentile_from_order_stats(cnt, [5, 95], lambda r: video.depthvis_select(db, r)[1])
        assert np.array_equal(got, want), (got, want)
    # refusals: nothing comes back
    with pytest.raises(ValueError):
        video.depthvis_select(db, (cnt,))
    with pytest.raises(ValueError):
        video.depthvis_select(db, (1, 0))


def test_depthvis_select_refusals_write_nothing():
    from unboundednerfpytorch_amd import _lib, video
    L = _lib.load()
    d, b = SETS["cnt65"]
    db = _dev(np.stack([d, b], axis=1))
    ws = torch.empty(int(L.ugrid_depthvis_select_ws_bytes()), dtype=torch.uint8, device="cuda")
    vals = (ctypes.c_float * 4)(*[-7.0] * 4)
    cnt = ctypes.c_int64(-5)
    st = _lib.stream_of(db)

    def call(ranks):
        r = (ctypes.c_int64 * len(ranks))(*ranks)
        return L.ugrid_depthvis_select(db.data_ptr(), db.shape[0], 0.1, len(ranks), ctypes.cast(r, ctypes.c_void_p), ctypes.addressof(cnt),
                                       ctypes.cast(vals, ctypes.c_void_p), ws.data_ptr(), st)
    assert call([5, 3]) == 1 and cnt.value == -5 and list(vals) == [-7.0] * 4            # unsorted: before any launch
    assert call([0, 65]) == 1 and cnt.value == 65 and list(vals) == [-7.0] * 4           # rank >= count: the count is known, no value written
    assert call([0, 64]) == 0 and cnt.value == 65 and list(vals)[2:] == [-7.0] * 2
    s = np.sort(vc.masked_values([d], [b]))
    assert list(vals)[:2] == [s[0], s[64]]
    # the threshold is an argument
    assert video.depthvis_select(db, (), thres=0.6)[0] == d.size and video.depthvis_select(db, (), thres=0.0)[0] == 0


# ------------------------------------------------------------------------------------------------------------------ ugrid_depth8_map
def _map_case(depth, bg, H, W, dmin, dmax, table, orientations):
    from unboundednerfpytorch_amd import video
    db = _dev(np.stack([depth.reshape(-1), bg.reshape(-1)], axis=1))
    tdev = _dev(table)
    for off, (flipy, k) in enumerate(orientations):
        want = vc.ref_depth8_map([depth.reshape(H, W, 1)], [bg.reshape(H, W, 1)], table, flipy=flipy, k=k, dmin=dmin, dmax=dmax)[0][0]
        buf, out = _byte_out(H * W * 3, off % 4)
        got = video.depth8_map(db, H, W, dmin, dmax, tdev, flipy, k, out=out)
        assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), (flipy, k)
        assert _sentinels_survive(buf, off % 4, H * W * 3)
    return want


@pytest.mark.parametrize("H,W", vc.SIZES + ((64, 4),))
def test_depth8_map_random_depths_with_numpy_percentiles(H, W):
    from unboundednerfpytorch_amd import video
    frame = _frame(H, W)
    _, depth, bg = vc.split(frame, H, W)
    vals = vc.masked_values([depth], [bg])
    dmin, dmax = np.percentile(vals, q=[5, 95]) if vals.size else (np.float64(3.0), np.float64(30.0))
    assert isinstance(dmin, np.float64)
    want = _map_case(depth, bg, H, W, dmin, dmax, video.rainbow_table(), vc.ORIENTATIONS if (H, W) != (64, 4) else [(False, 1)])
    assert H * W < 64 or len(np.unique(want.reshape(-1, 3), axis=0)) > 16
    table2 = np.random.RandomState(9).randint(0, 256, (256, 3)).astype(np.uint8)          # a second, arbitrary table
    _map_case(depth, bg, H, W, dmin, dmax, table2, [(False, 0), (True, 1)])


def test_depth8_map_bin_edges_and_degenerate_range():
    from unboundednerfpytorch_amd import video
    table = video.rainbow_table()
    j = np.arange(257, dtype=np.float32)                # dmin = 0, dmax = 256: t = j / 256 exactly
    depth = np.concatenate([j, np.nextafter(j, np.float32(-1)), np.nextafter(j, np.float32(300)), [-5.0, 300.0, np.nan, np.inf, -np.inf]]).astype(np.float32)
    H, W = 4, depth.size // 4
    assert H * W == depth.size
    bg = np.zeros(depth.size, np.float32)
    want = _map_case(depth, bg, H, W, 0.0, 256.0, table, [(False, 0), (False, 1)])
    assert want.shape == (W, H, 3)
    flat = vc.ref_depth8_map([depth.reshape(H, W, 1)], [bg.reshape(H, W, 1)], table, dmin=0.0, dmax=256.0)[0][0].reshape(-1, 3)
    assert np.array_equal(flat[0], table[255]) and np.array_equal(flat[256], table[0]) and np.array_equal(flat[128], table[128])
    # alphainv_last mixes in: v = d*(1 - b) + b in fp32
    bg2 = np.random.RandomState(4).uniform(0, 1, depth.size).astype(np.float32)
    _map_case(np.nan_to_num(depth, nan=1.0, posinf=7.0, neginf=-7.0), bg2, H, W, 0.0, 256.0, table, [(True, 3)])
    # dmax == dmin: (v - dmin) / 0 = +-inf or NaN -> the two ends of the table and the bad colour
    d3 = np.array([5.0, 4.0, 6.0, 5.0, np.nan, 7.5, 5.0, 1.0], np.float32)
    want3 = _map_case(d3, np.zeros(8, np.float32), 2, 4, 5.0, 5.0, table, [(False, 0), (True, 2)])
    flat3 = vc.ref_depth8_map([d3.reshape(2, 4, 1)], [np.zeros((2, 4, 1), np.float32)], table, dmin=5.0, dmax=5.0)[0][0].reshape(-1, 3)
    assert np.array_equal(flat3[0], [0, 0, 0]) and np.array_equal(flat3[1], table[255]) and np.array_equal(flat3[2], table[0])


# ------------------------------------------------------------------------------------------------------------------ end to end
def _reference_video(rgbs, depths, bgmaps, flipy, k, table, thres):
    """the literal lines of run_render.py on render_viewpoints' float frames (lists of [H,W,C])"""
    rgb8 = vc.ref_rgb8(rgbs, flipy, k)
    dmax8, dmax = vc.ref_depth8_max(depths, flipy, k)
    map8, dmin, dmaxp, n_masked = vc.ref_depth8_map(depths, bgmaps, table, thres=thres, flipy=flipy, k=k)
    return rgb8, dmax8, dmax, map8, dmin, dmaxp, n_masked


def _float_frames(rend, poses, HW, Ks, kw):
    """render_viewpoints view by view (it stacks its results, so one call takes one frame size)"""
    from unboundednerfpytorch_amd.run_render import render_viewpoints
    rgbs, depths, bgmaps = [], [], []
    for i in range(len(poses)):
        r, d, b = render_viewpoints(rend, poses[i:i + 1], HW[i:i + 1], Ks[i:i + 1], kw)
        rgbs.append(r[0]), depths.append(d[0]), bgmaps.append(b[0])
    return rgbs, depths, bgmaps


@pytest.mark.parametrize("name", ["dvgo", "fourier"])
def test_render_video_equals_the_reference_lines_on_render_viewpoints_frames(name):
    from unboundednerfpytorch_amd import video
    from unboundednerfpytorch_amd.run_render import render_video, render_viewpoints
    rend, kw = vc.make_renderer(name, torch.device("cuda:0"))
    table = video.rainbow_table()
    seen_masked = 0
    for sizes, stacked in ((((16, 24),) * 3, True), (((16, 24), (13, 7)), False)):
        poses, HW, Ks = vc.views(name, sizes)
        rgbs, depths, bgmaps = _float_frames(rend, poses, HW, Ks, kw)
        if stacked:                                     # the stacked call returns the same frames
            whole = render_viewpoints(rend, poses, HW, Ks, kw)
            assert all(np.array_equal(whole[0][i].view(np.int32), rgbs[i].view(np.int32)) for i in range(len(poses)))
        assert not np.array_equal(rgbs[0], rgbs[1]) and float(np.mean(bgmaps[0])) < 0.99
        for flipy, k in ((True, 1), (False, 0)):
            for thres in (0.1, 0.9):
                want_rgb, want_max, dmax, want_map, dmin, dmaxp, n_masked = _reference_video(rgbs, depths, bgmaps, flipy, k, table, thres)
                print("%s %s flipy=%s k=%d thres=%g: n_masked=%d dmax=%s dmin/dmax=%s/%s" % (name, sizes, flipy, k, thres, n_masked, dmax, dmin, dmaxp))
                seen_masked = max(seen_masked, n_masked)
                res = {}
                for fif in (1, 2):
                    common = dict(render_video_flipy=flipy, render_video_rot90=k, frames_in_flight=fif)
                    got = {None: render_video(rend, poses, HW, Ks, kw, **common),
                           "max": render_video(rend, poses, HW, Ks, kw, depth="max", **common),
                           "percentile": render_video(rend, poses, HW, Ks, kw, depth="percentile", bg_thres=thres, **common)}
                    for mode, (rgb8, depth8, info) in got.items():
                        assert isinstance(rgb8, np.ndarray if stacked else list) and len(rgb8) == len(poses)
                        assert all(a.dtype == np.uint8 and np.array_equal(a, w) for a, w in zip(rgb8, want_rgb)), (mode, fif)
                    assert got[None][1] is None and got[None][2] == {}
                    assert got["max"][2]["dmax"] == float(dmax)
                    assert all(np.array_equal(a, w) for a, w in zip(got["max"][1], want_max)) and len(got["max"][1]) == len(poses)
                    rgb8, depth8, info = got["percentile"]
                    assert info["n_masked"] == n_masked
                    if n_masked == 0:
                        assert depth8 is None
                    else:
                        assert info["dmin"] == dmin and info["dmax"] == dmaxp
                        assert len(depth8) == len(poses) and all(a.shape == w.shape and np.array_equal(a, w) for a, w in zip(depth8, want_map))
                    res[fif] = got
                for mode in res[1]:
                    assert all(np.array_equal(a, b) for a, b in zip(res[1][mode][0], res[2][mode][0]))
    assert seen_masked > 0                              # the percentile path really ran
    # an alternative colour map
    poses, HW, Ks = vc.views(name)
    table2 = np.random.RandomState(2).randint(0, 256, (256, 3)).astype(np.uint8)
    rgbs, depths, bgmaps = _float_frames(rend, poses, HW, Ks, kw)
    want = vc.ref_depth8_map(depths, bgmaps, table2, thres=0.9)[0]
    got = render_video(rend, poses, HW, Ks, kw, depth="percentile", bg_thres=0.9, colormap=table2)[1]
    assert np.array_equal(got, np.array(want))


def test_render_video_refuses_a_depth_buffer_beyond_free_memory():
    from unboundednerfpytorch_amd.run_render import render_video
    rend, kw = vc.make_renderer("dvgo", torch.device("cuda:0"))
    poses, HW, Ks = vc.views("dvgo")
    with pytest.raises(RuntimeError, match=r"%d bytes needed.* 1000 bytes are free" % (3 * 16 * 24 * 8)):
        render_video(rend, poses, HW, Ks, kw, depth="max", mem_get_info=lambda dev: (1000, 1 << 30))
    assert render_video(rend, poses, HW, Ks, kw, mem_get_info=lambda dev: (0, 0))[1] is None      # no depth mode: nothing kept


def test_render_video_percentile_without_a_pixel_under_the_threshold_gives_no_depth_video():
    """run_render.py:310-311: the reference prints a warning and writes no depth video; the colour frames still come back"""
    from unboundednerfpytorch_amd.run_render import render_video
    rend, kw = vc.make_renderer("dvgo", torch.device("cuda:0"))
    poses, HW, Ks = vc.views("dvgo")
    rgb8, depth8, info = render_video(rend, poses, HW, Ks, kw, depth="percentile", bg_thres=0.0)
    assert depth8 is None and info["n_masked"] == 0 and info["dmin"] is None
    assert np.array_equal(rgb8, render_video(rend, poses, HW, Ks, kw)[0]) and rgb8.shape == (3, 16, 24, 3)


WORKER = r'''
import os, sys
import numpy as np
import torch
import torch.distributed as dist
import video_cases as vc
outdir = sys.argv[1]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
local = int(os.environ["LOCAL_RANK"]) % torch.cuda.device_count()
torch.cuda.set_device(local)
dev = torch.device("cuda", local)
dist.init_process_group("gloo", rank=rank, world_size=world)
from unboundednerfpytorch_amd.run_render import render_video
rend, kw = vc.make_renderer("dvgo", dev)
poses, HW, Ks = vc.views("dvgo")
rgb8, depth8, info = render_video(rend, poses, HW, Ks, kw, render_video_flipy=True, render_video_rot90=1, depth="percentile", bg_thres=0.9, deal="tiles")
np.savez(os.path.join(outdir, "video_rank%d.npz" % rank), rgb8=rgb8, depth8=depth8, dmin=info["dmin"], dmax=info["dmax"], n_masked=info["n_masked"])
torch.cuda.synchronize()
dist.barrier()
if rank == 0:
    print("RESULT done")
dist.destroy_process_group()
'''


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_render_video_over_two_ranks_returns_the_single_process_bytes(tmp_path):
    """two gloo ranks sharing the GPU, launched as tests/test_gpu_frame_pipeline.py launches its ranks"""
    from unboundednerfpytorch_amd.run_render import render_video
    world = 2
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "video_worker.py")          # torch.distributed.run wants a script file
        with open(path, "w") as f:
            f.write(WORKER)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), path, str(tmp_path)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "RESULT done" in p.stdout, (p.stdout[-1500:], p.stderr[-3000:])
    rend, kw = vc.make_renderer("dvgo", torch.device("cuda:0"))
    poses, HW, Ks = vc.views("dvgo")
    rgb8, depth8, info = render_video(rend, poses, HW, Ks, kw, render_video_flipy=True, render_video_rot90=1, depth="percentile", bg_thres=0.9)
    assert info["n_masked"] > 0 and rgb8.shape == (3, 24, 16, 3) and depth8.shape == (3, 24, 16, 3)
    for rank in range(world):
        got = np.load(os.path.join(str(tmp_path), "video_rank%d.npz" % rank))
        assert np.array_equal(got["rgb8"], rgb8) and np.array_equal(got["depth8"], depth8), rank
        assert float(got["dmin"]) == info["dmin"] and float(got["dmax"]) == info["dmax"] and int(got["n_masked"]) == info["n_masked"]
