"""Host side of the video ops (no GPU needed): the rainbow table against its committed fixture (and matplotlib where it imports),
numpy's `linear` percentile from order statistics, the orientation plan of the library against np.flip / np.rot90, the entry
points' refusals before any launch, and the unit's kernels: compiled for gfx950 with no scratch and no spills."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import video_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ugrid_video_plan", "ugrid_frame_rgb8", "ugrid_depth8_max", "ugrid_depth8_map", "ugrid_depthvis_select_ws_bytes",
               "ugrid_depthvis_select")
EINVAL = 1      # hipErrorInvalidValue


def test_rainbow_table_equals_the_committed_fixture(golden_dir):
    from unboundednerfpytorch_amd import video
    t = video.rainbow_table()
    gold = np.load(os.path.join(golden_dir, "rainbow256.npy"))
    assert t.dtype == np.uint8 and t.shape == (256, 3) and gold.dtype == np.uint8
    assert np.array_equal(t, gold)
    assert len({tuple(r) for r in t}) > 200          # (a colour map, not a constant)


def test_rainbow_table_equals_matplotlib_for_all_256_entries():
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    from unboundednerfpytorch_amd import video
    cmap = plt.get_cmap('rainbow')
    x = (np.arange(256) + .5) / 256
    assert np.array_equal(video.rainbow_table(), vc.to8b(cmap(x)[..., :3]))
    # the lookup the test reference uses is matplotlib's: entry edges, both ends, beyond the ends after the clip, NaN
    xs = np.concatenate([np.arange(257) / 256.0, np.nextafter(np.arange(257) / 256.0, -1), [0.0, 1.0, np.nan], np.random.RandomState(0).uniform(0, 1, 500)])
    xs = np.clip(xs, 0, 1)
    assert np.array_equal(vc.lookup(video.rainbow_table(), xs), vc.to8b(cmap(xs)[..., :3]))


def _datasets(n, rs):
    yield "random", rs.uniform(-3, 40, n).astype(np.float32)
    yield "ties", rs.randint(0, 3, n).astype(np.float32) * np.float32(0.1)
    yield "equal", np.full(n, 1.7, np.float32)
    yield "wide", (rs.uniform(-1, 1, n) * np.exp2(rs.uniform(-30, 30, n))).astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 20, 21, 1000])
def test_percentile_from_order_stats_equals_numpy_exactly(n):
    from unboundednerfpytorch_amd import video
    rs = np.random.RandomState(n)
    qs = [0, 5, 50, 95, 100]
    for name, vals in _datasets(n, rs):
        s = np.sort(vals)
        calls = []

        def select(ranks):
            assert len(ranks) <= 4 and list(ranks) == sorted(ranks) and all(0 <= r < n for r in ranks)
            calls.append(list(ranks))
            return s[list(ranks)]
        for q in (qs, [5, 95], [50], [33.3, 99.9], np.array([2.5, 97.5])):
            want = np.percentile(vals, q=q)
            got = video.percentile_from_order_stats(n, q, select)
            assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, (name, q)
            assert np.array_equal(got, want), (name, q, got, want)
        del calls[:]
        video.percentile_from_order_stats(n, [5, 95], select)
        assert len(calls) == 1                      # the reference's q: one selection of at most four ranks
    with pytest.raises(ValueError):
        video.percentile_from_order_stats(0, [5], lambda r: [])
    with pytest.raises(ValueError):
        video.percentile_from_order_stats(3, [101], lambda r: [0.0] * len(r))


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (8, 8), (9, 13)])
def test_orientation_plan_is_flip_then_rot90(H, W):
    from unboundednerfpytorch_amd import video
    img = vc.index_image(H, W)
    for flipy in (False, True):
        for k in range(-1, 6):
            want = np.rot90(np.flip(img, 0) if flipy else img, k, axes=(0, 1))
            Ho, Wo, s0, si, sj = video.orientation(H, W, flipy, k)
            assert (Ho, Wo) == want.shape == video.out_shape(H, W, k), (flipy, k)
            i, j = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
            assert np.array_equal(s0 + i * si + j * sj, want), (flipy, k)


def test_entry_points_are_declared_exported_and_bound_with_the_abi_unchanged():
    import test_capi
    from unboundednerfpytorch_amd import _lib
    declared = test_capi.declared_functions()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS, name
    assert _lib.ABI_VERSION == 3 and _lib.load().ugrid_abi_version() == 3
    assert _lib.load().ugrid_depthvis_select_ws_bytes() == 4 * 2048 * 4


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """hipErrorInvalidValue from host checks alone (the pointers are never dereferenced: no device is present here)"""
    from unboundednerfpytorch_amd import _lib
    L = _lib.load()
    P = 4096
    plan = (ctypes.c_int64 * 5)()
    pp = ctypes.cast(plan, ctypes.c_void_p)
    assert L.ugrid_video_plan(3, 4, 0, 0, pp) == 0 and list(plan) == [3, 4, 0, 4, 1]
    for H, W in ((0, 4), (4, 0), (-1, 4), (1 << 31, 1), (1 << 16, 1 << 16)):
        assert L.ugrid_video_plan(H, W, 0, 0, pp) == EINVAL, (H, W)
    for H, W, stride in ((0, 8, 5), (8, 0, 5), (-3, 8, 5), (8, 8, 4), (8, 8, 0), (1 << 31, 1, 5), (1 << 15, 1 << 14, 5), (30000, 30000, 5)):
        assert L.ugrid_frame_rgb8(P, stride, H, W, 0, 0, P, None, None, None) == EINVAL, (H, W, stride)
    assert L.ugrid_frame_rgb8(None, 5, 8, 8, 0, 0, P, None, None, None) == EINVAL
    assert L.ugrid_frame_rgb8(P, 5, 8, 8, 0, 0, None, None, None, None) == EINVAL
    for H, W in ((0, 8), (8, -1), (1 << 31, 1), (1 << 16, 1 << 16)):
        assert L.ugrid_depth8_max(P, H, W, 0, 1, 1.0, P, None) == EINVAL
        assert L.ugrid_depth8_map(P, H, W, 0, 1, 0.0, 1.0, P, P, None) == EINVAL
    assert L.ugrid_depth8_map(P, 8, 8, 0, 0, 0.0, 1.0, None, P, None) == EINVAL          # no table
    ranks = (ctypes.c_int64 * 5)(0, 1, 2, 3, 4)
    vals = (ctypes.c_float * 5)(*[-7.0] * 5)
    cnt = ctypes.c_int64(-5)
    rp, vp, cp = ctypes.cast(ranks, ctypes.c_void_p), ctypes.cast(vals, ctypes.c_void_p), ctypes.addressof(cnt)
    assert L.ugrid_depthvis_select(P, 100, 0.1, 5, rp, cp, vp, P, None) == EINVAL           # m > 4
    assert L.ugrid_depthvis_select(P, 1 << 31, 0.1, 1, rp, cp, vp, P, None) == EINVAL       # n beyond 2^31 - 1
    assert L.ugrid_depthvis_select(P, -1, 0.1, 0, rp, cp, vp, P, None) == EINVAL
    unsorted = (ctypes.c_int64 * 2)(3, 1)
    assert L.ugrid_depthvis_select(P, 100, 0.1, 2, ctypes.cast(unsorted, ctypes.c_void_p), cp, vp, P, None) == EINVAL
    assert cnt.value == -5 and list(vals) == [-7.0] * 5                                        # nothing written
    assert L.ugrid_depthvis_select(None, 0, 0.1, 0, None, cp, None, None, None) == 0 and cnt.value == 0      # n == 0: no launch
    assert L.ugrid_depthvis_select(None, 0, 0.1, 1, rp, cp, vp, None, None) == EINVAL       # rank 0 >= count 0


def test_video_ops_refuse_host_tensors_before_any_library_call(monkeypatch):
    import torch
    from unboundednerfpytorch_amd import video
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        video.frame_rgb8(torch.zeros(64, 5), 8, 8)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        video.depth8_max(torch.zeros(64, 2), 8, 8, 1.0)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        video.depthvis_select(torch.zeros(64, 2), (0,))
    from unboundednerfpytorch_amd.run_render import render_video
    with pytest.raises(ValueError, match="depth"):
        render_video(None, [], [], [], {}, depth="median")


def test_kernels_compile_for_gfx950_without_scratch_or_spills():
    """the unit compiled alone with the library's flags and -Rpass-analysis=kernel-resource-usage: every kernel reports no scratch
    and no spilled register; the byte producers stay within 64 VGPRs (streaming kernels, 8 waves per SIMD)"""
    import tempfile
    csrc = os.path.join(ROOT, "unboundednerfpytorch_amd", "csrc")
    flags = re.search(r'^FLAGS="([^"]*)"', open(os.path.join(csrc, "build.sh")).read(), flags=re.M).group(1).split()
    assert "-ffp-contract=off" in flags and "--offload-arch=gfx950" in flags
    assert '"ugrid_video:"' in open(os.path.join(csrc, "build.sh")).read()          # no extra flags
    flags = [f.replace("../../include", os.path.join(ROOT, "include")) for f in flags]
    with tempfile.TemporaryDirectory() as td:
        p = subprocess.run(["hipcc"] + flags + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                            os.path.join(csrc, "ugrid_video.hip"), "-o", os.path.join(td, "v.o")], capture_output=True, text=True, cwd=csrc)
    assert p.returncode == 0, p.stderr[-3000:]
    kernels, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[bytes/lane\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    names = sorted(kernels)
    assert len([k for k in names if "k_video_bytes" in k]) == 3 and len([k for k in names if "k_select_hist" in k]) == 1, names
    for k in names:
        r = kernels[k]
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] <= 64, (k, r)
