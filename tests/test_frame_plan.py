"""dist.FramePlan / dist.FramePipeline on the host: the closed form that ugrid_frame_assemble evaluates per pixel against the table
built rank by rank from tile_assignment / shard_bounds, and the pipeline's exchange logic over gloo with a stand-in renderer."""
import multiprocessing as mp
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (8, 8): one tile, at world 8 seven ranks are empty; (13, 7): image order, ragged last tile; (9, 100): image order, 15 tiles --
# with deal_group 2 and 4 the last group is partial
SIZES = [(8, 8), (16, 24), (24, 40), (13, 7), (9, 100)]
WORLDS = [1, 2, 3, 8]
DEALS = [("bands", 0), ("tiles", 0), ("rows", 0), ("bands", 2), ("bands", 4)]


@pytest.mark.parametrize("deal,dg", DEALS)
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_source_row_is_the_table_and_a_permutation_onto_the_valid_rows(H, W, world, deal, dg):
    from unboundednerfpytorch_amd.dist import FramePlan, shard_bounds, tile_assignment
    plan = FramePlan(H, W, world, deal, dg)
    assert plan is FramePlan(H, W, world, deal, dg)                      # cached per key
    R = H * W
    assert plan.tile8 == (H % 8 == 0 and W % 8 == 0) and (plan.order is not None) == plan.tile8
    want_dg = dg if dg else {"bands": 0, "tiles": 1, "rows": max(1, W // 8)}[deal]
    assert plan.deal_group == want_dg
    # per and every rank's pixels: what render_sharded / bench.py derive from the two splitting functions
    if want_dg:
        shares = [tile_assignment(R, world, r, group=want_dg) for r in range(world)]
    else:
        shares = [torch.arange(*shard_bounds(R, world, r)) for r in range(world)]
    assert plan.per == shares[0].numel() == max(s.numel() for s in shares)
    assert sum(s.numel() for s in shares) == R
    valid = []
    for r in range(world):
        px = plan.px(r)
        assert torch.equal(px, shares[r] if plan.order is None else plan.order[shares[r]])
        # the closed form puts the k-th pixel of rank r at row r*per + k: a partial tile or group is the LAST of its owner's list
        assert torch.equal(plan.source_row(px), r * plan.per + torch.arange(px.numel()))
        valid.append(r * plan.per + torch.arange(px.numel()))
    src = plan.src_index()
    rows = plan.source_row(torch.arange(R))
    assert rows.dtype == torch.int64 and torch.equal(rows, src)
    assert torch.equal(torch.sort(rows).values, torch.cat(valid))          # a permutation onto the valid rows
    assert int(rows.max()) < world * plan.per and 5 * world * plan.per < 2 ** 31
    assert plan.source_row(R - 1) == src[R - 1]                            # a plain int works too
    if (H, W) == (8, 8) and world == 8:
        assert [plan.px(r).numel() for r in range(8)] == [64] + [0] * 7
    if (H, W) == (9, 100) and dg in (2, 4):
        n_tiles = -(-R // 64)
        assert n_tiles == 15 and n_tiles % dg != 0 and R % 64 != 0       # a partial last group that ends in a partial tile


def test_plan_arguments_are_checked():
    from unboundednerfpytorch_amd.dist import FramePlan
    with pytest.raises(ValueError):
        FramePlan(16, 24, 2, "columns")
    with pytest.raises(ValueError):
        FramePlan(16, 24, 0)
    assert FramePlan(16, 24, 2, "rows").deal_group == 3 and FramePlan(16, 24, 2, "rows", 5).deal_group == 5
    assert FramePlan(16, 24, 2, tile=0).tile8 is False                    # image order on request


def test_the_two_frame_symbols_are_exported():
    import __graft_entry__
    __graft_entry__.build()
    from unboundednerfpytorch_amd import _lib
    assert "ugrid_frame_pack" in _lib.EXPORTED_SYMBOLS and "ugrid_frame_assemble" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.ugrid_abi_version() == 3
    for name in ("ugrid_frame_pack", "ugrid_frame_assemble"):
        assert hasattr(lib, name)
    # refusals come before anything touches the device (no GPU here): sizes beyond 32-bit indexing, tile8 on an odd frame
    einval = 1
    assert lib.ugrid_frame_assemble(None, 8, 8, 8, 20726, 20726, 1, 64, 0, 0, 8, None) == einval
    assert lib.ugrid_frame_assemble(8, None, None, None, 13, 7, 1, 128, 0, 1, 8, None) == einval
    assert lib.ugrid_frame_assemble(8, None, None, None, 16, 24, 8, 1 << 26, 0, 1, 8, None) == einval
    assert lib.ugrid_frame_assemble(8, None, None, None, 16, 24, 2, 128, 0, 1, 8, None) == einval     # 2 * 128 rows < 384 pixels
    assert lib.ugrid_frame_assemble(8, None, None, None, 9, 100, 3, 320, 2, 0, 8, None) == einval     # rank 0's share is 384
    assert lib.ugrid_frame_pack(None, None, None, 1, 64, 8, None) == einval                           # n > 0 needs the arrays
    assert lib.ugrid_frame_pack(None, None, None, 0, 1 << 29, 8, None) == einval


class _StandIn:
    """FourierGridRenderer's forward signature on host tensors; a ray's outputs are single exact operations on that ray alone"""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def forward(self, o, d, v, stepsize=None, ray_order=None, render_depth=True):
        self.calls.append((int(o.shape[0]), ray_order))
        return {"rgb_marched": v * 3.0, "depth": o[:, 0] + d[:, 2], "alphainv_last": v[:, 1] * stepsize}


def _views():
    K = lambda H, W: [[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1]]
    out = []
    for i, (H, W) in enumerate([(16, 24), (13, 7), (16, 24), (13, 7)]):       # block order / image order, alternating
        c2w = torch.tensor([[1.0, 0, 0, 0.1 * i], [0, 0.8, 0.6, -0.2], [0, -0.6, 0.8, 0.3 + 0.05 * i]])
        out.append((H, W, K(H, W), c2w))
    return out


def _frames(pipe):
    got = [pipe.submit(H, W, K, c2w, stepsize=0.5) for H, W, K, c2w in _views()] + [pipe.flush()]
    return got


def _single_process_frames():
    from unboundednerfpytorch_amd.dist import FramePipeline
    model = _StandIn()
    pipe = FramePipeline(model)
    got = _frames(pipe)
    assert pipe.world == 1 and got[4] is None and all(f is not None for f in got[:4])
    assert [c[1] for c in model.calls] == ["coherent", "auto", "coherent", "auto"]
    return got[:4]


def test_single_process_frames_are_the_image_order_render():
    from unboundednerfpytorch_amd.fourier_render import get_rays_of_a_view
    frames = _single_process_frames()
    for (H, W, K, c2w), f in zip(_views(), frames):
        o, d, v = [x.reshape(-1, 3) for x in get_rays_of_a_view(H, W, K, c2w)]
        want = _StandIn().forward(o, d, v, stepsize=0.5)
        assert f.shape == (H * W, 5)
        assert torch.equal(f, torch.cat([want["rgb_marched"], want["depth"][:, None], want["alphainv_last"][:, None]], 1))
    assert not torch.equal(frames[0], frames[2])                            # the poses differ


def _pipeline_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from unboundednerfpytorch_amd.dist import FramePipeline
    res = {}
    for deal, dg in DEALS:
        model = _StandIn()
        pipe = FramePipeline(model, deal=deal, deal_group=dg)
        got = _frames(pipe)
        assert got[0] is None and pipe.flush() is None                      # view k comes back from submit k + 1, the last from flush
        res[(deal, dg)] = ([f.numpy().copy() for f in got[1:]], sum(n for n, _ in model.calls))
    q.put((rank, res))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 8])
def test_pipeline_over_gloo_returns_the_single_process_frames_on_every_rank(world):
    """four consecutive views alternating between two frame sizes (plans and buffers change, both gathered buffers are re-used), every
    deal; 13 x 7 at world 8 leaves six ranks without rays, which still take part in every collective"""
    import queue
    import socket
    import time
    import numpy as np
    want = [f.numpy() for f in _single_process_frames()]
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_pipeline_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, t_end = [], time.time() + 240
    try:
        while len(res) < world:
            try:
                res.append(q.get(timeout=2))
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead and time.time() < t_end, "rank(s) died (exit codes %s) or timed out" % dead
        for p in procs:
            p.join(30)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert sorted(r for r, _ in res) == list(range(world))
    n_rays = sum(H * W for H, W, _, _ in _views())
    for deal, dg in DEALS:
        assert sum(r[(deal, dg)][1] for _, r in res) == n_rays              # every ray rendered once, on one rank
        for rank, r in res:
            frames = r[(deal, dg)][0]
            assert len(frames) == 4
            for f, w in zip(frames, want):
                assert np.array_equal(f.view(np.int32), w.view(np.int32)), (rank, deal, dg)
