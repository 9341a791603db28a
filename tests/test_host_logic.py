"""CPU tests of the host-side logic around the kernels: sample tables, sharding, the 2-rank exchange."""
import os
import sys

import numpy as np
import pytest
import types

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import model_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_table_matches_oracle():
    from unboundednerfpytorch_amd.fourier_render import sample_table
    for world_len, stepsize in ((200, 0.5), (200, 1.31), (300, 0.5), (16, 0.7)):
        t, s = sample_table(world_len, stepsize, 0.2)
        t_ref = model_oracle.sample_t(world_len, stepsize, 0.2)
        assert torch.equal(t, t_ref)
        assert torch.equal(s, 1 - 1 / (1 + t_ref))
    assert sample_table(200, 1.31, 0.2)[0].numel() == 256   # S1: N_inner = N_outer = 128
    assert sample_table(200, 0.5, 0.2)[0].numel() == 668    # garden_single.py


def test_shard_bounds_cover_and_align():
    from unboundednerfpytorch_amd.dist import shard_bounds
    for n in (0, 1, 63, 64, 65, 1000, 2073600):
        for ws in (1, 2, 3, 8):
            spans = [shard_bounds(n, ws, r) for r in range(ws)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            for (b0, e0), (b1, e1) in zip(spans, spans[1:]):
                assert e0 == b1
            for b, e in spans:
                if e < n:  # every shard that is not the tail is a whole number of 64-ray wave tiles
                    assert (e - b) % 64 == 0
    assert shard_bounds(2073600, 8, 3) == (3 * 259200, 4 * 259200)


WORLDS = (2, 3, 8)      # every collective path runs at an even, an odd and the node's full world size (VERDICT r4 "missing" #2)


def _spawn(target, world, port, *extra, timeout=300):
    """start `world` gloo ranks of `target(rank, world, port, *extra, q)` and return their queue items sorted by rank.  The
    rendezvous port is one the OS reports free right now (`port` is only a hint kept for readability: pid-derived ports collided
    with sockets of earlier tests still in TIME_WAIT)"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(extra) + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    import queue
    import time
    res, t_end = [], time.time() + timeout
    while len(res) < world:
        try:
            res.append(q.get(timeout=2))
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or time.time() > t_end:          # a rank that raised never reports: fail NOW, do not wait for the others' time-outs
                for p in procs:
                    p.kill()
                raise AssertionError("rank(s) died (exit codes %s) or timed out; got %d of %d results" % (dead, len(res), world))
    for p in procs:
        p.join(timeout=60)
    return sorted(res, key=lambda t: t[0])


def _fake_forward(o, d, v, **kw):
    # stands in for FourierGridRenderer.forward on CPU: any per-ray function works for the exchange logic
    rgb = torch.stack([o[:, 0] + d[:, 0], o[:, 1] * 2, v[:, 2] - 1], dim=1)
    return {"rgb_marched": rgb, "depth": o.sum(-1), "alphainv_last": d.sum(-1)}


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    from unboundednerfpytorch_amd.dist import render_sharded
    ok = True
    for R in (1000, 64, 7, 129, 64 * world + 1):          # ragged tile counts: ranks with a short share, ranks with NO rays
        g = torch.Generator().manual_seed(3 + R)
        o, d, v = [torch.randn(R, 3, generator=g) for _ in range(3)]
        out = render_sharded(_fake_forward, o, d, v, stepsize=0.5)
        ref = _fake_forward(o, d, v)
        ok = ok and all(torch.equal(out[k], ref[k]) for k in ref)
    q.put((rank, ok))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", WORLDS)
def test_render_sharded_gloo(world):
    res = _spawn(_worker, world, 29500 + (os.getpid() + 17 * world) % 2000)
    assert res == [(r, True) for r in range(world)]


# ---------------------------------------------------------------------------------------------------------
# ShardedMaskedAdam: per-voxel Adam state sharded over the ranks (reduce-scatter -> shard update -> all-gather).
# CPU / gloo, with the oracle's Adam kernels injected as the update back-end (the HIP ones need a GPU); the
# result must equal a single-process run of the same kernels on the rank-averaged gradient, bit for bit.
# ---------------------------------------------------------------------------------------------------------
def _adam_case(seed, world=2):
    """per-rank gradients on a 2^-8 lattice with |g| < 4: the sum over <= 8 ranks is EXACT in fp32, so the collectives' summation
    order (gloo's / RCCL's ring order depends on the chunking) cannot show -- the single-process reference below is a same-value
    sum for every world size, and equality can be asserted bit for bit at world 3 and 8, not only at 2"""
    g = torch.Generator().manual_seed(seed)
    shapes = {"k0": (7, 4, 6, 6, 6), "dens": (7, 1, 5, 6, 5), "w": (16, 9)}   # 6048 (exact split), 1050 (padded), 144
    params = {k: torch.randn(s, generator=g) for k, s in shapes.items()}
    grads = []
    for step in range(3):
        per_rank = []
        for r in range(world):
            d = {}
            for k, s in shapes.items():
                x = (torch.randn(s, generator=g).clamp(-3.9, 3.9) * 256).round() / 256
                if k != "w":
                    x = torch.where(torch.rand(s, generator=g) < 0.2, x, torch.zeros(s))   # sparse grid gradients
                d[k] = x
            per_rank.append(d)
        grads.append(per_rank)
    return params, grads


def _adam_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from oracle import ref_ops
    from unboundednerfpytorch_amd.sharded_adam import ShardedMaskedAdam
    params, grads = _adam_case(11, world)
    rank_mean = lambda step, k: sum(grads[step][r][k] for r in range(world)) * (1.0 / world)   # exact sum, ONE rounding (the scale)
    P = {k: torch.nn.Parameter(v.clone()) for k, v in params.items()}
    # the training layout of multi-channel grids: the same logical tensor stored channel-last; its flat shards follow the
    # STORAGE order, the result must be the same logical tensor (Adam is elementwise)
    cl = lambda t: t.clone().contiguous(memory_format=torch.channels_last_3d)
    P["k0cl"] = torch.nn.Parameter(cl(params["k0"]))
    opt = ShardedMaskedAdam([{'params': [P["k0"], P["dens"], P["k0cl"]], 'lr': 0.1, 'skip_zero_grad': True},
                             {'params': [P["w"]], 'lr': 1e-3, 'skip_zero_grad': False}],
                            min_shard_numel=512, ops=ref_ops)
    for step in range(3):
        for k in P:
            P[k].grad = cl(grads[step][rank]["k0"]) if k == "k0cl" else grads[step][rank][k].clone()
        if step == 1:
            P["k0cl"].grad = grads[step][rank]["k0"].clone()      # a row-major gradient for a channel-last parameter
        opt.step()
    # single-process reference: the same kernels on the rank-averaged gradient with full-size state
    R = {k: v.clone() for k, v in params.items()}
    M = {k: torch.zeros_like(v) for k, v in R.items()}
    V = {k: torch.zeros_like(v) for k, v in R.items()}
    for step in range(3):
        for k in R:
            gsum = rank_mean(step, k)
            fn = ref_ops.adam_upd if k == "w" else ref_ops.masked_adam_upd
            fn(R[k], gsum, M[k], V[k], step + 1, 0.9, 0.99, 1e-3 if k == "w" else 0.1, 1e-8)
    ok = all(torch.equal(P[k].data, R[k]) for k in R)
    ok = ok and torch.equal(P["k0cl"].data, R["k0"]) and not P["k0cl"].data.is_contiguous() \
        and P["k0cl"].data.is_contiguous(memory_format=torch.channels_last_3d)
    m_cl, v_cl = opt.gather_full_state(P["k0cl"])
    ok = ok and torch.equal(m_cl, M["k0"]) and torch.equal(v_cl, V["k0"])
    sd = opt.state_dict()                                   # collective; the reference's full-shape layout
    ok = ok and torch.equal(sd['state'][2]['exp_avg'], M["k0"]) and tuple(sd['state'][2]['exp_avg'].shape) == tuple(R["k0"].shape)
    # ... and loads back into a fresh sharded optimizer over channel-last / row-major parameters alike: one more step on
    # both optimizers gives identical parameters
    import copy
    P2 = {k: torch.nn.Parameter(v.data.clone(memory_format=torch.preserve_format)) for k, v in P.items()}
    opt2 = ShardedMaskedAdam([{'params': [P2["k0"], P2["dens"], P2["k0cl"]], 'lr': 0.1, 'skip_zero_grad': True},
                              {'params': [P2["w"]], 'lr': 1e-3, 'skip_zero_grad': False}], min_shard_numel=512, ops=ref_ops)
    opt2.load_state_dict(copy.deepcopy(sd))
    for PP, oo in ((P, opt), (P2, opt2)):
        for k in PP:
            PP[k].grad = cl(grads[0][rank]["k0"]) if k == "k0cl" else grads[0][rank][k].clone()
        oo.step()
    ok = ok and all(torch.equal(P[k].data, P2[k].data) for k in P) and torch.equal(P2["k0cl"].data, P2["k0"].data)
    for k in R:                                             # (the reference run follows with the same fourth step)
        gsum = rank_mean(0, k)
        fn = ref_ops.adam_upd if k == "w" else ref_ops.masked_adam_upd
        fn(R[k], gsum, M[k], V[k], 4, 0.9, 0.99, 1e-3 if k == "w" else 0.1, 1e-8)
    ok = ok and all(torch.equal(P[k].data, R[k]) for k in R)
    m_full, v_full = opt.gather_full_state(P["dens"])
    ok = ok and torch.equal(m_full, M["dens"]) and torch.equal(v_full, V["dens"])
    # state memory really is sharded: k0's moments live only for this rank's 1 / world of the flat range
    ok = ok and opt.state[P["k0"]]['exp_avg'].numel() == ShardedMaskedAdam.shard_len(P["k0"].numel(), world) < P["k0"].numel()
    ok = ok and opt.state[P["w"]]['exp_avg'].shape == P["w"].shape
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", WORLDS)
def test_sharded_masked_adam_gloo(world):
    """reduce-scatter -> shard update -> all-gather over 2, 3 and 8 gloo ranks equals the single-process optimizer on the rank-mean
    gradient BIT FOR BIT (exactly representable sums: see _adam_case), incl. padded tails (1050 elements over 3 / 8 ranks), the
    channel-last layout, checkpoints through the full-shape state_dict"""
    res = _spawn(_adam_worker, world, 31500 + (os.getpid() + 17 * world) % 2000)
    assert res == [(r, True) for r in range(world)]


def test_sharded_masked_adam_single_process_equals_plain_loop():
    """Without a process group the optimizer degenerates to MaskedAdam's loop (full state, no collectives)."""
    from oracle import ref_ops
    from unboundednerfpytorch_amd.sharded_adam import ShardedMaskedAdam
    params, grads = _adam_case(5)
    p = torch.nn.Parameter(params["dens"].clone())
    opt = ShardedMaskedAdam([{'params': [p], 'lr': 0.1, 'skip_zero_grad': True}], ops=ref_ops)
    r, m, v = params["dens"].clone(), torch.zeros_like(params["dens"]), torch.zeros_like(params["dens"])
    for step in range(2):
        p.grad = grads[step][0]["dens"].clone()
        opt.step()
        ref_ops.masked_adam_upd(r, grads[step][0]["dens"], m, v, step + 1, 0.9, 0.99, 0.1, 1e-8)
    assert torch.equal(p.data, r)
    assert ShardedMaskedAdam.shard_len(1050, 2) == 528 and ShardedMaskedAdam.shard_len(6048, 8) == 756


def test_step_param_updates_one_parameter_early_and_step_skips_it():
    """ShardedMaskedAdam.step_param (what the post-accumulate-grad hook of train_iteration calls for the k0 grid): the parameter
    is updated exactly once per iteration -- by step_param, with its TV term -- and the following step() handles the others"""
    from oracle import ref_ops
    from unboundednerfpytorch_amd.sharded_adam import ShardedMaskedAdam
    params, grads = _adam_case(7)
    tv = types.SimpleNamespace(total_variation_add_grad=ref_ops.total_variation_add_grad)

    def run(early):
        a = torch.nn.Parameter(params["k0"].clone())
        b = torch.nn.Parameter(params["dens"].clone())
        opt = ShardedMaskedAdam([{'params': [a, b], 'lr': 0.1, 'skip_zero_grad': True}], ops=ref_ops)
        for step in range(2):
            a.grad, b.grad = grads[step][0]["k0"].clone(), grads[step][0]["dens"].clone()
            terms = {a: (1e-3, step == 0, tv), b: (2e-3, False, tv)}
            if early:
                assert opt.step_param(a, terms[a], overlap=False) is True
            opt.step(tv_terms=terms)
        assert opt.state[a]['step'] == 2 and opt.state[b]['step'] == 2
        return a.detach().clone(), b.detach().clone()
    (a1, b1), (a0, b0) = run(True), run(False)
    assert torch.equal(a1, a0) and torch.equal(b1, b0)
    p = torch.nn.Parameter(params["dens"].clone())
    opt = ShardedMaskedAdam([{'params': [p], 'lr': 0.1, 'skip_zero_grad': True}], ops=ref_ops)
    assert opt.step_param(p) is False                                  # no gradient: nothing done
    q = torch.nn.Parameter(params["dens"].clone()); q.grad = torch.ones_like(q)
    assert opt.step_param(q) is False                                  # not one of the optimizer's parameters


def test_touched_line_bitmap_is_bound_to_buffer_and_backward():
    """_gradpool.touch_for_backward / touch_of (host logic of the touched-line bitmap): bitmaps exist only for parameters the
    training step has CERTIFIED for the running backward (the buffer address alone does not prove that nothing else
    contributed to .grad); one bitmap per gradient buffer, served only for the very tensor the single marking backward filled,
    dropped when marking is off"""
    from unboundednerfpytorch_amd import _gradpool
    lib = types.SimpleNamespace(ugrid_touch_words=lambda n: ((n + 63) // 64 + 31) // 32)
    _gradpool.clear()
    try:
        p = torch.nn.Parameter(torch.zeros(3, 4, 5, 6, 7))
        key = id(p)
        buf = torch.zeros_like(p)
        assert _gradpool.touch_for_backward(key, buf, lib) is None        # not certified: no bitmap, nothing is marked
        p.grad = buf
        assert _gradpool.touch_of(p, p.grad) is None
        _gradpool.certify([p])
        t = _gradpool.touch_for_backward(key, buf, lib)
        assert t.dtype == torch.int32 and t.numel() == ((p.numel() + 63) // 64 + 31) // 32 and not bool(t.any())
        assert _gradpool.touch_of(p, p.grad) is t
        assert _gradpool.touch_for_backward(key, buf, lib) is t           # a SECOND marking backward in the same step ...
        assert _gradpool.touch_of(p, p.grad) is None                      # ... voids the bitmap (.grad is a sum of two scatters)
        _gradpool.certify([p])                                            # next step: the same buffer comes back from the pool
        assert _gradpool.touch_for_backward(key, buf, lib) is t and _gradpool.touch_of(p, p.grad) is t      # same bitmap
        other = torch.zeros_like(p)
        assert _gradpool.touch_of(p, other) is None                       # not .grad
        p.grad = other
        assert _gradpool.touch_of(p, p.grad) is None                      # .grad is another buffer (accumulated, user-made)
        _gradpool.certify([p])
        t2 = _gradpool.touch_for_backward(key, other, lib)                 # a backward into a fresh buffer: new bitmap
        assert t2 is not t and _gradpool.touch_of(p, p.grad) is t2
        p.grad = buf
        assert _gradpool.touch_of(p, p.grad) is None                      # the first buffer's bitmap is gone with it
        _gradpool.decertify([p])
        p.grad = other
        assert _gradpool.touch_of(p, p.grad) is None                      # the step is over: the certificate is spent
        _gradpool.certify([p])
        _gradpool.touch_enabled = False
        assert _gradpool.touch_of(p, other) is None and _gradpool.touch_for_backward(key, other, lib) is None
        _gradpool.touch_enabled = True
        assert _gradpool.touch_of(p, p.grad) is None                      # an unmarked backward invalidated the bitmap
        assert _gradpool.touch_for_backward(key, other, lib) is not None and _gradpool.touch_of(p, p.grad) is None   # and the certificate
        assert _gradpool.touch_for_backward(None, buf, lib) is None       # not a poolable parameter
    finally:
        _gradpool.touch_enabled = True
        _gradpool.clear()


def test_rgbnet_features_on_the_host_is_the_reference_chain():
    """ops.rgbnet_features with CPU tensors (the models' CPU forward): the reference's expressions, FourierGrid_model.py:631-635"""
    from unboundednerfpytorch_amd import ops
    torch.manual_seed(3)
    viewdirs = torch.nn.functional.normalize(torch.randn(6, 5, 3), dim=-1)
    viewfreq = torch.tensor([1.0, 2.0, 4.0, 8.0])
    ray_id = torch.tensor([0, 0, 3, 29, 29, 29])
    k0 = torch.randn(6, 12)
    e = (viewdirs.unsqueeze(-1) * viewfreq).flatten(-2)
    emb = torch.cat([viewdirs, e.sin(), e.cos()], -1).flatten(0, -2)
    assert torch.equal(ops.rgbnet_features(None, viewdirs, viewfreq, None), emb)
    assert torch.equal(ops.rgbnet_features(None, viewdirs, viewfreq, ray_id), emb[ray_id])
    assert torch.equal(ops.rgbnet_features(k0, viewdirs, viewfreq, ray_id), torch.cat([k0, emb[ray_id]], -1))
    rows = ops.ViewRows(viewdirs, viewfreq, ray_id)
    assert isinstance(rows, tuple) and rows[0] is viewdirs and rows[2] is ray_id


@pytest.mark.parametrize("mode", ["fourier", "dvgo", "dcvgo"])
def test_native_step_host_side_runs_over_a_stand_in_library(mode, monkeypatch):
    """native_step.VoxGOStep's host side -- input checks, struct fill for the three modes, buffer sizing after the one host read,
    the returned arrays' shapes, and BOTH backward routes (all gradients returned; or the k0 gradient assigned and handed to the
    `k0_grad_ready` callback between the two halves, the node then reporting none for k0) -- with the C entry points replaced by a
    stand-in that only fills M1 / M2, on CPU tensors, incl. strided views as ray inputs.  The kernels' results are the GPU tests'
    business (test_gpu_voxgo_train.py, test_gpu_train_scale.py)."""
    import ctypes
    from unboundednerfpytorch_amd import _lib, native_step, voxgo_model as vm
    from unboundednerfpytorch_amd.fourier_model import FourierGridModel
    calls = []

    class StandIn:
        def ugrid_voxgo_step_sample(self, ps, st):
            s = ctypes.cast(ps, ctypes.POINTER(_lib.VoxgoStep)).contents
            assert s.mode == {"dvgo": 0, "dcvgo": 1, "fourier": 2}[mode] and s.n_rays == 8 and s.C == 12 and s.pe == 4 and s.width == 128
            assert (s.P, s.kP, s.freq_num) == ((5, 5, 2) if mode == "fourier" else (1, 1, 0))
            assert bool(s.mask) == (mode != "fourier") and bool(s.t_table) == (mode != "dvgo") and s.slots == (20 if mode == "dvgo" else 16)
            s.M1, s.M2 = 40, 17
            calls.append("sample")
            return 0

        def ugrid_voxgo_step_ws_floats(self, ps):
            return 1000

        def ugrid_voxgo_step_bwd_ws_floats(self, ps):
            return 1000

        def __getattr__(self, name):
            if name.startswith("ugrid_voxgo_step_"):
                def f(ps, st, _n=name[len("ugrid_voxgo_step_"):]):
                    s = ctypes.cast(ps, ctypes.POINTER(_lib.VoxgoStep)).contents
                    assert s.ws and s.logits and s.weights2 and (_n == "forward" or (s.grad_loss and s.ws_bwd and s.grad_k0_grid and s.g_w2))
                    calls.append(_n)
                    return 0
                return f
            if name == "ugrid_touch_words":
                return lambda n: (n + 2047) // 2048
            raise AttributeError(name)

    monkeypatch.setattr(native_step, "_L", StandIn())
    monkeypatch.setattr(_lib, "require_cuda", lambda *a: None)
    monkeypatch.setattr(_lib, "require_cuda_grid", lambda *a: _lib.is_channels_last(a[0][1]))
    monkeypatch.setattr(_lib, "stream_of", lambda t: None)
    monkeypatch.setattr(_lib, "guard", lambda d: _lib._NO_GUARD)
    monkeypatch.setattr(_lib, "empty_like_grid", lambda shape, cl, dev, zero=False: torch.zeros(shape).contiguous(
        memory_format=torch.channels_last_3d if cl else torch.contiguous_format))
    R = 8
    if mode == "fourier":
        m = FourierGridModel(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels_density=10 ** 3, num_voxels_base_density=10 ** 3,
                             num_voxels_rgb=10 ** 3, num_voxels_base_rgb=10 ** 3, num_voxels_viewdir=-1, alpha_init=1e-4, fast_color_thres=1e-4,
                             fourier_freq_num=2, rgbnet_dim=12)
        cfg = {"act_shift": 0.0, "interval": 0.5, "thres": 1e-4, "scene_center": [0., 0., 0.], "scene_radius": [1., 1., 1.], "bg_len": 0.2,
               "norm_l2": False, "freq_num": 2, "k0_freq_num": 2}
        t, bg, mask = torch.linspace(0, 1, 16), None, None
    else:
        kw = dict(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=12 ** 3, num_voxels_base=12 ** 3, alpha_init=1e-2, fast_color_thres=1e-4,
                  rgbnet_dim=12)
        m = vm.DirectVoxGO(rgbnet_direct=True, **kw) if mode == "dvgo" else vm.DirectContractedVoxGO(**kw)
        cfg = {"act_shift": 0.0, "interval": 0.5, "thres": 1e-4, "mask_scale": [1., 1., 1.], "mask_shift": [0., 0., 0.]}
        cfg.update({"near": 0.2, "far": 1e9, "stepdist": 0.1, "slots": 20} if mode == "dvgo" else
                   {"scene_center": [0., 0., 0.], "scene_radius": [1., 1., 1.], "bg_len": 0.2, "norm_l2": False, "dist_thres": 0.01})
        t, bg, mask = (None if mode == "dvgo" else torch.linspace(0, 1, 16)), torch.rand(R, 3), m.mask_cache.mask
    params = m._native_params()

    def pack():
        return {"mode": mode, "cfg": cfg, "t": t, "rays_o": torch.zeros(R, 3), "rays_d": torch.ones(R, 6)[:, ::2], "viewdirs": torch.ones(3, R).t(),
                "viewfreq": m.viewfreq, "xyz_min": m.xyz_min, "xyz_max": m.xyz_max, "k0_xyz_min": m.k0.xyz_min, "k0_xyz_max": m.k0.xyz_max,
                "mask": mask, "target": torch.zeros(R, 3), "bg": bg, "coef": (1, 0, 0, 0, 0, 0, 0.1, R)}
    pk = pack()
    loss, mse = native_step.VoxGOStep.apply(*params, pk)
    assert loss.requires_grad and not mse.requires_grad and loss.shape == mse.shape == ()
    out = pk["out"]
    assert out["weights"].shape == out["ray_id"].shape == (17,) and out["raw_logits"].shape == (17, 3) and out["loss_mse"].shape == (2,)
    assert out["alphainv_last"].shape == (R,) and out["rgb_marched"].shape == (R, 3) and (out["inner"] is None) == (mode != "dcvgo")
    loss.backward()
    assert all(p.grad is not None and p.grad.shape == p.shape for p in params)
    assert calls == ["sample", "forward", "backward"]
    # the mid-backward route: the callback sees the k0 gradient assigned, the node returns none for k0
    del calls[:]
    for p in params:
        p.grad = None
    pk = pack()
    seen = []
    pk["k0_grad_ready"] = lambda prm: seen.append((prm is m.k0.grid, prm.grad is not None))
    native_step.VoxGOStep.apply(*params, pk)[0].backward()
    assert seen == [(True, True)] and calls == ["sample", "forward", "backward_k0", "backward_density"]
    assert m.k0.grid.grad is not None and m.density.grid.grad is not None
    # ... and not over a gradient that is already accumulated (it has to be ADDED by autograd then)
    del calls[:], seen[:]
    pk = pack()
    pk["k0_grad_ready"] = lambda prm: seen.append(1)
    native_step.VoxGOStep.apply(*params, pk)[0].backward()
    assert seen == [] and calls[-1] == "backward"
    with pytest.raises(RuntimeError, match=r"\[R,3\]"):
        bad = pack()
        bad["target"] = torch.zeros(R + 1, 3)
        native_step.VoxGOStep.apply(*params, bad)


def test_native_step_selection_is_host_logic():
    """Which configurations take native_step.VoxGOStep is decided on the host from the module's own state (no device needed): the
    default 3-layer rgbnet fed by all of k0, every parameter trainable, gradients on, the HIP lookups (no injected query function);
    residual-colour and coarse-stage models, frozen parameters, no_grad and injected back-ends select the op-by-op ops."""
    from unboundednerfpytorch_amd import voxgo_model as vm
    from unboundednerfpytorch_amd.fourier_model import FourierGridModel
    kw = dict(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=12 ** 3, num_voxels_base=12 ** 3, alpha_init=1e-2, fast_color_thres=1e-4)
    direct = vm.DirectVoxGO(rgbnet_dim=12, rgbnet_direct=True, **kw)
    p = direct._native_params()
    assert p is not None and len(p) == 8 and p[0] is direct.density.grid and p[1] is direct.k0.grid
    assert vm.DirectVoxGO(rgbnet_dim=9, rgbnet_direct=False, **kw)._native_params() is None            # residual colour
    assert vm.DirectVoxGO(rgbnet_dim=0, **kw)._native_params() is None                                 # coarse stage: no rgbnet
    assert vm.DirectVoxGO(rgbnet_dim=12, rgbnet_direct=True, rgbnet_depth=4, **kw)._native_params() is None      # not the default network
    with torch.no_grad():
        assert direct._native_params() is None
    direct.k0.grid.requires_grad_(False)
    assert direct._native_params() is None
    direct.k0.grid.requires_grad_(True)
    direct.native_step = False
    assert direct._native_params() is None
    dc = vm.DirectContractedVoxGO(rgbnet_dim=12, **kw)
    assert dc._native_params() is not None
    fg = dict(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels_density=10 ** 3, num_voxels_base_density=10 ** 3, num_voxels_rgb=10 ** 3,
              num_voxels_base_rgb=10 ** 3, num_voxels_viewdir=-1, alpha_init=1e-4, fast_color_thres=1e-4, fourier_freq_num=2, rgbnet_dim=12)
    m = FourierGridModel(**fg)
    p = m._native_params()
    assert p is not None and p[0].shape[0] == 5 and p[1].shape[0] == 5
    import types
    be = types.SimpleNamespace(Raw2Alpha=None, Alphas2Weights=None, grid_query=lambda *a: None, total_variation_cuda=None, render_utils_cuda=None)
    assert FourierGridModel(backend=be, **fg)._native_params() is None                                   # injected back-end: op-by-op


def test_rgbnet_linears_recognises_only_the_default_network():
    from unboundednerfpytorch_amd import ops
    nn = torch.nn
    ok = nn.Sequential(nn.Linear(39, 128), nn.ReLU(inplace=True), nn.Sequential(nn.Linear(128, 128), nn.ReLU(inplace=True)), nn.Linear(128, 3))
    lin = ops.rgbnet_linears(ok)
    assert lin is not None and [l.in_features for l in lin] == [39, 128, 128] and lin[2].out_features == 3
    narrow = nn.Sequential(nn.Linear(36, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 3))               # free_dataset: width 64
    assert [l.out_features for l in ops.rgbnet_linears(narrow)] == [64, 64, 3]
    for bad in (nn.Sequential(nn.Linear(39, 64), nn.ReLU(), nn.Linear(64, 3)),                                  # depth 2
                nn.Sequential(nn.Linear(39, 256), nn.ReLU(), nn.Linear(256, 256), nn.ReLU(), nn.Linear(256, 3)),    # wider than 128
                nn.Sequential(nn.Linear(39, 64), nn.ReLU(), nn.Linear(64, 128), nn.ReLU(), nn.Linear(128, 3)),      # unequal widths
                nn.Sequential(nn.Linear(39, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 3)),
                nn.Sequential(nn.Linear(39, 128), nn.Sigmoid(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 3)),   # another activation
                nn.Sequential(nn.Linear(39, 128, bias=False), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 3)),
                nn.Sequential(nn.Linear(200, 128), nn.ReLU(), nn.Linear(128, 128), nn.ReLU(), nn.Linear(128, 3))):    # input wider than 128
        assert ops.rgbnet_linears(bad) is None


# ---------------------------------------------------------------------------------------------------------
# interleaved tile dealing and block compositing (dist.py), 2 ranks over gloo
# ---------------------------------------------------------------------------------------------------------
def _block_forward(block):
    def fwd(o, d, v, **kw):
        rgb = torch.sigmoid(torch.stack([o[:, 0] + block, d[:, 1] * (block + 1), v[:, 2]], dim=1))
        # odd blocks are (nearly) transparent for these rays: they fail the opacity rule
        last = torch.sigmoid(o.sum(-1) * (3.0 if block % 2 == 0 else 0.5) + (4.0 if block % 2 == 1 else -1.0))
        return {"rgb_marched": rgb, "depth": d.abs().sum(-1) + block, "alphainv_last": last}
    return fwd


def _block_rule(outs, dists, min_op, p=4.0):
    """single-process evaluation of the merging rule (eval_block_nerf.py:95-133,215-225) in float64: blocks with mean visibility
    <= min_opacity are dropped, the others blended with normalised distance^-p weights; when none is left the reference skips the
    frame -- composite_blocks then returns the inverse-distance blend of all blocks"""
    nb = len(outs)
    vis = [float((1 - outs[b]["alphainv_last"]).mean()) > min_op for b in range(nb)]
    dmin = min(dists)
    ws_ = [((dists[b] / dmin) ** -p) if (vis[b] or not any(vis)) else 0.0 for b in range(nb)]
    tot = sum(ws_)
    want = {k: sum(outs[b][k].double() * ws_[b] for b in range(nb)) / tot for k in ("rgb_marched", "depth", "alphainv_last")}
    return want, [w / tot for w in ws_], vis


def _distn_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    from unboundednerfpytorch_amd.dist import composite_blocks, render_sharded, tile_assignment
    ok = True
    fails = []
    for R in (1000, 64, 7, 200, 129, 64 * world + 1):
        g = torch.Generator().manual_seed(R)
        o, d, v = [torch.randn(R, 3, generator=g) for _ in range(3)]
        out = render_sharded(_fake_forward, o, d, v, interleave=True, stepsize=0.5)
        ref = _fake_forward(o, d, v)
        fails.append(1) if not (all(torch.equal(out[k], ref[k]) for k in ref)) else None
        allidx = torch.cat([tile_assignment(R, world, r) for r in range(world)])
        fails.append(2) if not (sorted(allidx.tolist()) == list(range(R))) else None  # every ray dealt exactly once
    # blocks: rank b holds block b (world blocks)
    g = torch.Generator().manual_seed(5)
    R = 300
    o, d, v = [torch.randn(R, 3, generator=g) for _ in range(3)]
    cam = torch.tensor([0.5, -0.2, 0.1])
    cents = [torch.tensor([1.0 + 0.7 * b, 0.3 * ((-1) ** b) * b, 0.5 * (b % 3)]) for b in range(world)]
    outs = [_block_forward(b)(o, d, v) for b in range(world)]
    dists = [float((cam.double() - c.double()).norm()) for c in cents]
    for min_op in (0.05, 0.0, 2.0):
        for how in ("all_centroids", "min_collective", "ref_distance"):
            kw = {"all_centroids": cents} if how == "all_centroids" else ({"ref_distance": 0.75} if how == "ref_distance" else {})
            got = composite_blocks(_block_forward(rank), o, d, v, cam, cents[rank], p=4.0, min_opacity=min_op, **kw)
            want, wn, vis = _block_rule(outs, dists, min_op)
            for k in want:
                fails.append(3) if not (torch.allclose(got[k].double(), want[k], rtol=1e-5, atol=1e-6)) else None
            fails.append(4) if not (abs(float(got["block_weight"]) - wn[rank]) <= 1e-6 and int(got["visible_blocks"]) == sum(vis)) else None
        if min_op == 0.05:
            fails.append(5) if not (vis == [b % 2 == 0 for b in range(world)]) else None  # the case really exercises the visibility rule
        if min_op == 2.0:
            fails.append(6) if not (not any(vis)) else None
    # un-centred, city-scale coordinates: cameras 1e4 ... 1e5 units from every centroid.  The absolute weights are
    # 1e-16 ... 1e-20 (x 2^-60 for an invisible block: denormal), the RATIOS are ordinary numbers and must survive
    cam_far = torch.tensor([3.0e4, -7.0e4, 1.0e3])
    cents_far = [torch.tensor([1.0e3 * (b + 1), 2.0e3 * b, -5.0e2 * b]) for b in range(world)]
    dists_far = [float((cam_far.double() - c.double()).norm()) for c in cents_far]
    fails.append(7) if not (min(dists_far) > 1.0e4) else None
    for how in ("all_centroids", "min_collective"):
        kw = {"all_centroids": cents_far} if how == "all_centroids" else {}
        got = composite_blocks(_block_forward(rank), o, d, v, cam_far, cents_far[rank], p=4.0, min_opacity=0.0, **kw)
        want, wn, vis = _block_rule(outs, dists_far, 0.0)          # (every block visible: the ratios decide the blend)
        fails.append(8) if not (abs(float(got["block_weight"]) - wn[rank]) <= 1e-6 * max(wn)) else None
        fails.append(9) if not (len({round(w, 9) for w in wn if w > 0}) > 1) else None  # the weights really differ between the blocks
        for k in want:
            fails.append(10) if not (torch.allclose(got[k].double(), want[k], rtol=1e-5, atol=1e-6)) else None
    q.put((rank, not fails, fails))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", WORLDS)
def test_interleaved_sharding_and_block_compositing_gloo(world):
    """tile dealing (every ray exactly once, ragged counts, ranks without rays) and `composite_blocks` with `world` blocks over
    2, 3 and 8 gloo ranks: the three ways of agreeing on the weight scale, the visibility rule, and city-scale camera distances"""
    res = _spawn(_distn_worker, world, 33500 + (os.getpid() + 17 * world) % 2000)
    assert res == [(r, True, []) for r in range(world)], res


def test_bench_parity_stats_fields():
    """bench.py's gpu_vs_oracle block: pure host arithmetic over per-ray errors and threshold margins."""
    import bench
    err = torch.tensor([1e-6, 2e-5, 5e-7, 1.5e-4, 3e-6])
    margin = torch.tensor([0.5, 2e-3, 5e-5, 3e-2, float("inf")])
    st = bench.parity_stats(err, margin, sq_rgb=5 * 3 * 1e-10)
    assert st["rays"] == 5 and abs(st["linf_all"] - 1.5e-4) < 1e-10
    assert abs(st["frac_rays_above_1e-5"] - 0.4) < 1e-6
    assert abs(st["psnr_rgb_db"] - 100.0) < 1e-6                      # mse 1e-10 -> 100 dB
    assert abs(st["linf_margin_gt_0.0001"] - 1.5e-4) < 1e-10 and abs(st["frac_rays_margin_gt_0.0001"] - 0.8) < 1e-6
    assert abs(st["linf_margin_gt_0.01"] - 1.5e-4) < 1e-10 and abs(st["frac_rays_margin_gt_0.01"] - 0.6) < 1e-6
    st2 = bench.parity_stats(err[:3], margin[:3], sq_rgb=1.0)
    assert abs(st2["linf_margin_gt_0.01"] - 1e-6) < 1e-10
    assert "note" in st


# ---------------------------------------------------------------------------------------------------------
# data-parallel training: 2 ranks (gloo), each with half of the ray batch and ShardedMaskedAdam, against the
# single-process step on the whole batch (model = fourier_model.FourierGridModel with the oracle back-end)
# ---------------------------------------------------------------------------------------------------------
def _dp_setup():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import synth
    import test_fourier_model as T
    c = dict(synth.MODEL_UTILS_CASE, dm=0.5, ds=2.0)
    cfg = dict(T.TRAIN_CFG, weight_main=1.0, weight_entropy_last=0.001, weight_tv_density=1e-4, weight_tv_k0=1e-5, tv_after=0,
               tv_before=10, tv_every=1, tv_dense_before=2,     # step 1 dense TV, step 2 masked TV
               weight_nearclip=0.01, weight_distortion=0.01, weight_rgbper=0.05)   # sum-type and ray-normalised terms
    o, d, v = [torch.from_numpy(a) for a in synth.rays(77, 128)]
    target = torch.sigmoid(torch.from_numpy(synth.normal(78, 128 * 3).reshape(128, 3)))
    return T, c, cfg, (o, d, v, target)


NEAR_THRES = 0.35   # t < NEAR_THRES: the samples the nearclip term pushes on (a few per ray at stepsize 0.5)


def _dp_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    from oracle import ref_ops
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.sharded_adam import ShardedMaskedAdam
    from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model
    T, c, cfg, (o, d, v, target) = _dp_setup()
    m = T.build(c)
    opt = create_optimizer_or_freeze_model(m, cfg, 0, sharded=True, ops=ref_ops)
    opt.min_shard_numel = 256
    assert isinstance(opt, ShardedMaskedAdam)
    sl = slice(rank * 64, (rank + 1) * 64)
    # (a) the loss scaling alone: gradient of training_loss(world_size=2) on the half batch, averaged over the ranks
    dfn = T.model_oracle_distortion()
    out = m(o[sl], d[sl], v[sl], global_step=1, is_train=True, stepsize=0.5)
    last_ray_sampled = int(out['ray_id'].max()) + 1 == 64
    loss, _ = ts.training_loss(out, target[sl], cfg, 64, near_thres=NEAR_THRES, distortion_fn=dfn, world_size=world)
    loss.backward()
    avg = {}
    for k, p in m.named_parameters():
        g = p.grad.clone()
        dist.all_reduce(g)
        avg[k] = (g / world).numpy().copy()
        p.grad = None
    # (b) two full iterations
    for step in (1, 2):
        ts.train_iteration(m, opt, o[sl], d[sl], v[sl], target[sl], cfg, step, dict(stepsize=0.5), world_size=world,
                           near_thres=NEAR_THRES, distortion_fn=dfn)
    params_after_2 = {k: p.detach().numpy().copy() for k, p in m.named_parameters()}     # numpy: pickled by value
    shard_numel = opt.state[m.k0.grid]['exp_avg'].numel()
    # (c) checkpoint round trip: state_dict() is the reference's full-shape layout on every rank; a fresh
    # sharded optimizer that loads it continues bit-identically to the one that kept running
    import copy
    sd = opt.state_dict()
    k0_index = [i for i, p in enumerate(pp for g in opt.param_groups for pp in g['params']) if p is m.k0.grid][0]
    full_ok = (tuple(sd['state'][k0_index]['exp_avg'].shape) == tuple(m.k0.grid.shape)
               and all('shard' not in st for st in sd['state'].values()))
    sd_np = {i: {k: (x.numpy().copy() if torch.is_tensor(x) else x) for k, x in st.items()} for i, st in sd['state'].items()}
    m2 = T.build(c)
    m2.load_state_dict(m.state_dict())
    m2.act_shift = m.act_shift
    opt2 = create_optimizer_or_freeze_model(m2, cfg, 0, sharded=True, ops=ref_ops)
    opt2.min_shard_numel = 256
    opt2.load_state_dict(copy.deepcopy(sd))
    for g2, g1 in zip(opt2.param_groups, opt.param_groups):
        assert g2['lr'] == g1['lr']
    resumed_sharded = opt2.state[m2.k0.grid]['exp_avg'].numel() == shard_numel
    for mm, oo in ((m, opt), (m2, opt2)):
        ts.train_iteration(mm, oo, o[sl], d[sl], v[sl], target[sl], cfg, 3, dict(stepsize=0.5), world_size=world,
                           near_thres=NEAR_THRES, distortion_fn=dfn)
    same = all(torch.equal(a, b) for a, b in zip(m.parameters(), m2.parameters()))
    q.put((rank, params_after_2, shard_numel, avg, last_ray_sampled, full_ok and resumed_sharded and same, sd_np))
    dist.destroy_process_group()


def test_data_parallel_training_matches_single_process_gloo():
    from oracle import ref_ops
    from unboundednerfpytorch_amd import train_step as ts
    from unboundednerfpytorch_amd.train_utils import create_optimizer_or_freeze_model
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + os.getpid() % 2000
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    # single process, whole batch
    torch.set_num_threads(1)
    T, c, cfg, (o, d, v, target) = _dp_setup()
    m = T.build(c)
    opt = create_optimizer_or_freeze_model(m, cfg, 0, ops=ref_ops)
    # (a) whole-batch gradient of the same loss: the rank-averaged half-batch gradients must equal it (ADVICE r1:
    # nearclip is a SUM over samples -> x world_size in data-parallel mode; distortion / rgbper are ray-normalised)
    dfn = T.model_oracle_distortion()
    out = m(o, d, v, global_step=1, is_train=True, stepsize=0.5)
    assert int((out['t'] < NEAR_THRES).sum()) > 50 and res[0][4] and res[1][4]     # the terms are really exercised
    loss, _ = ts.training_loss(out, target, cfg, 128, near_thres=NEAR_THRES, distortion_fn=dfn)
    loss.backward()
    for k, p in m.named_parameters():
        want = p.grad.numpy()
        scale = float(np.abs(want).max())
        assert scale > 0, k
        assert np.array_equal(res[0][3][k], res[1][3][k]), k
        np.testing.assert_allclose(res[0][3][k], want, rtol=0, atol=2e-5 * scale, err_msg=k)
        p.grad = None
    # and a wrong scaling would be seen: dropping the x world_size of nearclip changes the density gradient by > 10 %
    for step in (1, 2):
        ts.train_iteration(m, opt, o, d, v, target, cfg, step, dict(stepsize=0.5), near_thres=NEAR_THRES, distortion_fn=dfn)
    ref = {k: p.detach() for k, p in m.named_parameters()}
    for k in ref:
        assert np.array_equal(res[0][1][k], res[1][1][k]), k                   # the ranks stay in lock-step
        diff = (torch.from_numpy(res[0][1][k]) - ref[k]).abs()
        lr = 0.1 if 'grid' in k else 1e-3
        # the mean-of-halves gradient equals the whole-batch gradient up to summation order; Adam's first steps move
        # an entry by ~lr whatever its gradient's size, so compare against a fraction of one step
        assert float((diff > 0.05 * lr).float().mean()) < 5e-3, (k, float(diff.max()))
    assert res[0][2] == m.k0.grid.numel() // 2                                 # k0's Adam state is split over the ranks
    # checkpoint round trip: full-shape state on both ranks, identical, loads into the single-process MaskedAdam (the
    # reference optimizer's layout) and matches that optimizer's own state after the same two steps
    assert res[0][5] and res[1][5]
    mine = opt.state_dict()
    plist = [pp for g in opt.param_groups for pp in g['params']]
    for i, st in mine['state'].items():
        name = [n for n, pp in m.named_parameters() if pp is plist[i]][0]
        for k in ('exp_avg', 'exp_avg_sq'):
            assert np.array_equal(res[0][6][i][k], res[1][6][i][k])
            assert res[0][6][i][k].shape == tuple(st[k].shape)
            if 'grid' in name:
                # (the rgbnet's second-step gradient depends on first-step Adam moves of +-lr whose sign is decided by
                # gradients at rounding level, so only the grids' moments are compared value by value)
                scale = float(st[k].abs().max())
                bad = np.abs(res[0][6][i][k] - st[k].numpy()) > 1e-2 * scale
                assert bad.mean() < 5e-3, (name, k, float(bad.mean()))
        assert res[0][6][i]['step'] == st['step'] == 2
    loaded = {'state': {i: {k: (torch.from_numpy(x) if isinstance(x, np.ndarray) else x) for k, x in st.items()}
                        for i, st in res[0][6].items()}, 'param_groups': mine['param_groups']}
    opt.load_state_dict(loaded)
    assert opt.state[m.k0.grid]['exp_avg'].shape == m.k0.grid.shape


# ---------------------------------------------------------------------------------------------------------
# bench.py's strong-scaled step (one frame over N ranks + the tile all-gather) over gloo, with a stand-in renderer
# ---------------------------------------------------------------------------------------------------------
from bench_standin import Renderer as _FakeRenderer  # noqa: E402  (per-ray outputs = a function of the ray alone)


def _bench_worker(rank, world, port, contiguous, hw, dg, q):
    import argparse
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    import bench
    args = argparse.Namespace(height=hw[0], width=hw[1], grid=200, contiguous=contiguous, pipeline=0, mlp_mode=None,
                              ray_tile=8, deal="rows", deal_group=dg)       # dg = 0: block rows; > 0: groups of dg tiles
    fb = bench.FrameBench(args, None, torch.device("cpu"), world, rank, dist, renderer=_FakeRenderer())
    assert (fb.order is not None) == (hw[0] % 8 == 0 and hw[1] % 8 == 0)
    dt, timing = fb.timed(3, 1)
    fb.check_exchange()
    frame = fb.assembled_frame()
    rays = sum(n for _, n in timing) // 3
    q.put((rank, frame.numpy().copy(), rays, dt > 0))
    dist.destroy_process_group()


@pytest.mark.parametrize("world,contiguous,hw,dg", [(2, False, (37, 101), 1), (2, True, (37, 101), 1), (2, False, (40, 104), 1), (2, True, (40, 104), 1),
                                                    (3, False, (40, 104), 1), (3, True, (37, 101), 1), (8, False, (40, 104), 1), (8, True, (40, 104), 1),
                                                    (8, False, (16, 24), 1), (2, False, (40, 104), 0), (8, False, (40, 104), 0), (3, False, (40, 104), 4)])
def test_bench_strong_scaled_step_over_gloo(world, contiguous, hw, dg):
    """the frame every rank assembles INSIDE the timed step (un-deal / un-band + un-tile of the 8 x 8 pixel-block ray order:
    one index_select) is the single-process frame in image order -- 2, 3 and 8 ranks, ragged shares, (16 x 24 pixels = 6 tiles
    over 8 ranks) ranks that render nothing, tiles dealt singly (dg = 1), by block rows of the image (dg = 0) and in groups of 4;
    contiguous = the bench's default bands"""
    import argparse
    import bench
    res = _spawn(_bench_worker, world, 37500 + (os.getpid() + 17 * world + (1 if contiguous else 0) + hw[0] + 3 * dg) % 2000, contiguous, hw, dg)
    args = argparse.Namespace(height=hw[0], width=hw[1], grid=200, contiguous=contiguous, pipeline=0, mlp_mode=None,
                              ray_tile=0)
    fb = bench.FrameBench(args, None, torch.device("cpu"), 1, 0, None, renderer=_FakeRenderer())
    ro, rd, vd = fb.rays()                    # image order
    want = _FakeRenderer()(ro, rd, vd)
    R = hw[0] * hw[1]
    for rank, frame, rays, ok in res:
        assert ok and frame.shape == (R, 5)
        np.testing.assert_array_equal(frame[:, 0:3], want["rgb_marched"].numpy())
        np.testing.assert_array_equal(frame[:, 3], want["depth"].numpy())
        np.testing.assert_array_equal(frame[:, 4], want["alphainv_last"].numpy())
    shares = [r[2] for r in res]
    assert sum(shares) == R                                     # every ray rendered once
    if not contiguous and dg == 1:
        assert max(shares) - min(shares) <= 64                  # dealt tiles: balanced to ONE 64-ray tile
    if not contiguous and dg == 0 and hw[1] % 8 == 0:
        assert max(shares) - min(shares) <= 8 * hw[1]           # dealt block rows: balanced to one 8-pixel-high row of the image


def test_bench_launches_itself_for_n_gt_1(tmp_path):
    """`python bench.py --gpus 2` with no launcher in the environment (how the driver starts the N = 1 line, with N = 2):
    bench.py re-executes itself through torch.distributed.run on 127.0.0.1 and rank 0 prints the ONE JSON line.  CI runs it
    with the CPU stand-in renderer over gloo (UGRID_BENCH_STANDIN); on a GPU box the same path runs the HIP renderer."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["UGRID_BENCH_STANDIN"] = "bench_standin:Renderer"
    env["OMP_NUM_THREADS"] = "1"
    detail = str(tmp_path / "bench_detail.json")
    env["UGRID_BENCH_DETAIL"] = detail
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--height", "40",
                        "--width", "104", "--full"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    assert len(lines[0]) < 4096                 # the driver parses this line: round 5's 22 KB line was recorded as unparsed
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["steps"] == 2 and res["scaling"] == "strong"
    assert res["assembled_frame_equals_single_rank_frame"] is True and "stand-in" in res["renderer"]
    assert "frame assembly" in res["config"]["step"] and res["weak_scaling"]["value"] > 0
    # everything else is in the detail file the line names (path relative to the repo root + sha16 of its bytes)
    import hashlib
    blob = open(detail, "rb").read()
    assert res["detail"]["sha16"] == hashlib.sha256(blob).hexdigest()[:16] and res["detail"]["bytes"] == len(blob)
    full = json.loads(blob)
    assert sum(r["rays"] for r in full["per_rank"]) == 40 * 104 and full["value"] == pytest.approx(res["value"], rel=1e-4)
    # a wrong launcher environment is refused, not silently run at another size
    env2 = dict(env, WORLD_SIZE="3", RANK="0")
    p2 = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env2, capture_output=True, text=True, timeout=120)
    assert p2.returncode != 0 and "WORLD_SIZE=3" in (p2.stderr + p2.stdout)


@pytest.mark.parametrize("gpus,extra", [(1, []), (2, []), (1, ["--shuffle-rays"])])
def test_bench_plain_run_prints_the_headline_and_dumps_the_last_frame(tmp_path, gpus, extra):
    """A plain run (no --full) times exactly --steps steps after --warmup ones, prints the headline keys and nothing it did not measure,
    writes no detail file, and --dump-outputs DIR holds the frame of the LAST timed step in image order (N = 2: the frame assembled from
    both ranks' tiles; --shuffle-rays: put back from the shuffled order) -- the same arrays run after run.  The CPU stand-in's depth
    carries the number of renderer calls so far: the dumped frame must be call warmup + steps on every rank."""
    import argparse
    import json
    import subprocess
    import bench_standin
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["UGRID_BENCH_STANDIN"] = "bench_standin:CountingRenderer"
    env["OMP_NUM_THREADS"] = "1"
    env["UGRID_BENCH_DETAIL"] = str(tmp_path / "bench_detail.json")
    H, W = 40, 104
    dumps = []
    for rep, (steps, warmup) in enumerate(((3, 1), (3, 1), (2, 3))):
        d = tmp_path / ("out%d" % rep)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", str(steps), "--warmup", str(warmup),
                            "--height", str(H), "--width", str(W), "--dump-outputs", str(d)] + extra,
                           env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout[-2000:]
        res = json.loads(lines[0])
        for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup"):
            assert k in res, k
        assert res["steps"] == steps and res["warmup"] == warmup and res["n_gpus"] == gpus and res["ms_per_step"] > 0
        assert res["value"] == pytest.approx(H * W * res["config"]["samples_per_ray"] / (res["ms_per_step"] * 1e-3) / 1e6, rel=1e-4)
        for k in ("kernels", "roofline", "cpu_baseline", "weak_scaling", "detail", "secondary_ms", "scaling_proxy_N8"):
            assert k not in res, k
        dumps.append((warmup + steps, {n: np.load(str(d / (n + ".npy"))) for n in ("rgb_marched", "depth", "alphainv_last")}))
    assert not (tmp_path / "bench_detail.json").exists()
    import bench
    args = argparse.Namespace(height=H, width=W, grid=200, contiguous=False, pipeline=0, mlp_mode=None, ray_tile=0)
    fb = bench.FrameBench(args, None, torch.device("cpu"), 1, 0, None, renderer=_FakeRenderer())
    rays = fb.rays()                    # image order
    for calls, got in dumps:
        want = bench_standin.CountingRenderer()
        want.calls = calls - 1
        want = want(*rays)              # = call number `calls`
        for n in ("rgb_marched", "depth", "alphainv_last"):
            assert got[n].dtype == np.float32
            np.testing.assert_array_equal(got[n], want[n].numpy())
    for n in dumps[0][1]:
        np.testing.assert_array_equal(dumps[0][1][n], dumps[1][1][n])


def test_bench_dump_samples_a_frame_beyond_the_budget(tmp_path, monkeypatch):
    """--dump-outputs of a frame larger than DUMP_BUDGET: within the budget, the same fixed, seeded rows of every output -- each
    sampled row is the stand-in's output for the ray of that pixel, in every array."""
    import argparse
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    H, W = 40, 104
    args = argparse.Namespace(height=H, width=W, grid=200, contiguous=False, pipeline=0, mlp_mode=None, ray_tile=8)
    fb = bench.FrameBench(args, None, torch.device("cpu"), 1, 0, None, renderer=_FakeRenderer())
    fb.timed(1, 0)
    img = bench.FrameBench(argparse.Namespace(**dict(vars(args), ray_tile=0)), None, torch.device("cpu"), 1, 0, None, renderer=_FakeRenderer())
    want = _FakeRenderer()(*img.rays())                    # image order
    g = torch.Generator()
    g.manual_seed(0)
    rows = torch.randperm(H * W, generator=g)[:4000 // 20].sort().values       # 20 bytes per ray: rgb 3 + depth + alphainv_last, fp32
    blobs = []
    for rep in range(2):
        bench.dump_outputs(fb, str(tmp_path / str(rep)))
        got = {n: np.load(str(tmp_path / str(rep) / (n + ".npy"))) for n in ("rgb_marched", "depth", "alphainv_last")}
        assert sum(v.nbytes for v in got.values()) <= 4000
        for n, v in got.items():
            np.testing.assert_array_equal(v, want[n][rows].numpy())
        blobs.append(open(str(tmp_path / str(rep) / "rgb_marched.npy"), "rb").read())
    assert blobs[0] == blobs[1]


def test_bench_line_fits_the_driver(tmp_path):
    """the ONE line stays under 4 KB whatever the run measured -- checked on the largest result bench.py has ever
    produced (round 5's 22 KB line, profiles/r05/bench_s1_line.json) -- carries every key of the contract plus `roofline` and
    `cpu_baseline` as numbers (no prose), one number per secondary, and names the detail file that holds the rest."""
    import json
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r05", "bench_s1_line.json")))
    assert len(json.dumps(full)) > 20000
    line = bench.compact_line(full, str(tmp_path / "d.json"))
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < bench.LINE_BUDGET == 4096 and "\n" not in text
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline", "kernels", "detail"):
        assert k in line, k
    assert len(line["config"]["workload"]) < 120 and set(line["kernels"]) == {"render_march", "render_shade"}
    rf = line["roofline"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "ta_busy_measured", "hbm_frac_measured", "frac_of_hbm_algorithmic"):
        assert k in rf, k
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and rf["frac"] == pytest.approx(full["roofline"]["frac"], rel=1e-3)
    assert not any(isinstance(v, str) and len(v) > 24 for v in rf.values())            # numbers and names only
    assert line["roofline_hbm"]["frac"] == pytest.approx(full["roofline_hbm"]["frac"], rel=1e-3)
    cb = line["cpu_baseline"]
    assert cb["kind"] in ("reference", "port") and cb["cores"] == 8 and cb["value"] > 0 and set(cb["linf"]) == {"rgb", "depth", "alphainv_last"}
    sec = line["secondary_ms"]
    assert sec["truck_render"] == pytest.approx(full["secondary_truck_render"]["ms_per_step"], rel=1e-3)
    assert sec["dvgo_lego_fine"] > 0 and sec["s3_train_masked_tv"] > 0 and sec["s1b_s668_render"] > 0
    assert json.load(open(tmp_path / "d.json")) == full
    # a result bloated far past anything real still prints a parseable line: optional blocks are dropped, the contract's keys never
    fat = dict(full, secondary_voxgo_train_steps={("leg%03d" % i): {"ms_per_step": 1.0 + i} for i in range(400)})
    line2 = bench.compact_line(fat, str(tmp_path / "d2.json"))
    assert len(json.dumps(line2, separators=(",", ":"))) < 4096 and "roofline" in line2 and "cpu_baseline" in line2 and "secondary_ms" not in line2


def test_device_code_hash_ignores_the_non_loaded_sections(tmp_path):
    """bench.device_code_sha16 = sha256 of .hip_fatbin: two builds of the same device code whose files differ only in
    .comment / .symtab / .strtab (what happened between the profiling box and the driver's box in round 2) hash alike."""
    import bench
    from unboundednerfpytorch_amd import _lib
    a = bench.device_code_sha16()
    assert a is not None and len(a) == 16
    blob = bytearray(open(_lib.LIB_PATH, "rb").read())
    off, sec = bench.elf_section(_lib.LIB_PATH, ".comment", with_offset=True)
    assert len(sec) > 4
    blob[off] = blob[off] ^ 0x20
    other = tmp_path / "lib_copy.so"
    other.write_bytes(bytes(blob))
    import hashlib
    assert hashlib.sha256(bytes(blob)).hexdigest()[:16] != bench.lib_sha16()
    assert bench.device_code_sha16(str(other)) == a


def test_roofline_block_merges_counters_only_for_the_same_device_code(tmp_path, monkeypatch):
    """bench.roofline_block: static PMC counters (profiles/r05/pmc_summary.json) are merged only when they were taken on
    the SAME device code (sha256 of .hip_fatbin); otherwise the block says so and carries live times + algorithmic rates
    only.  The algorithmic-bytes-over-HBM-peak figure is printed, labelled, and never chosen as the bound; the measured
    L1 peak of the micro-benchmark is used when its file is there; a rank's share scales the per-frame counters."""
    import json
    import bench
    code = bench.device_code_sha16()
    R, S, M = 2073600, 256, 26065245
    kern = {"render_march": 4.3, "render_shade": 4.5}
    pmc = {"device_code_sha16": code,
           "render_march": {"hbm_bytes": 6.2e9, "valu_insts": 3.65e9, "mfma_busy_cycles": 0.0, "gui_active_cycles": 9.4e6},
           "render_shade": {"hbm_bytes": 6.7e9, "valu_insts": 1.2e9, "mfma_busy_cycles": 3.5e9, "gui_active_cycles": 9.2e6}}
    monkeypatch.setattr(bench, "PROFILE_DIR", str(tmp_path))
    # 1. no files at all
    r = bench.roofline_block(kern, M, R, S, M // 32)
    assert r["traffic"] is None and r["pmc_source"] is None and r["pmc_refused"] is None
    assert r["frame"]["frac_of_hbm_algorithmic"] > 1.0 and r["bound"] in ("l1", "mfma") and 0 < r["frac"] < 1
    assert "cache-served" in r["per_kernel"]["render_march"]["frac_of_hbm_algorithmic_note"]
    assert r["per_kernel"]["render_shade"]["mfma_useful_TFLOPs"] < r["per_kernel"]["render_shade"]["mfma_TFLOPs"]
    # 2. counters of this very device code + the L1 calibration
    (tmp_path / "pmc_summary.json").write_text(json.dumps(pmc))
    (tmp_path / "microbench_l1_dwordx4.json").write_text(json.dumps({"quad64_B_per_clk_per_CU": 61.6, "linear_B_per_clk_per_CU": 63.8}))
    r = bench.roofline_block(kern, M, R, S, M // 32)
    assert r["pmc_refused"] is None and r["pmc_device_code_sha16"] == code
    # the summary entry is ALWAYS the kernel with the lower fraction of its roof (round 4: no 5 % window) -- the shade here --, says
    # so, and carries the > 1 algorithmic-over-HBM figure WITH its warning next to the measured HBM fraction
    assert r["kernel"] == "render_shade" and "LOWER" in r["kernel_choice"] and r["traffic"] == 6.7e9
    assert r["frac_of_hbm_algorithmic"] > 1.0 and "NOT a roofline fraction" in r["frac_of_hbm_algorithmic_note"]
    assert abs(r["hbm_frac_measured"] - 6.7e9 / 4.5e-3 / 1e9 / 8000.0) < 1e-9
    assert abs(r["frame"]["hbm_bytes_pmc"] - 12.9e9) < 1e6
    sh = r["per_kernel"]["render_shade"]
    assert abs(sh["hbm_frac"] - 6.7e9 / 4.5e-3 / 1e9 / 8000.0) < 1e-9 and 0.3 < sh["mfma_pipe_busy"] < 0.45
    assert abs(sh["l1_frac_of_measured_peak"] / sh["l1_frac"] - 64.0 / 61.6) < 1e-9
    assert r["peaks"]["l1_B_per_clk_per_CU_measured"]["quad_64B_gather"] == 61.6
    # 3. a rank's half of the frame: counters scaled by its share
    r2 = bench.roofline_block({k: v / 2 for k, v in kern.items()}, M // 2, R // 2, S, M // 64, frame_rays=R)
    assert r2["pmc_scaled_to_rank_share"] == 0.5 and abs(r2["per_kernel"]["render_shade"]["hbm_bytes_pmc"] - 3.35e9) < 1e3
    # 4. counters of ANOTHER build: refused, nothing merged
    (tmp_path / "pmc_summary.json").write_text(json.dumps(dict(pmc, device_code_sha16="0123456789abcdef")))
    r = bench.roofline_block(kern, M, R, S, M // 32)
    assert r["traffic"] is None and "0123456789abcdef" in r["pmc_refused"] and "hbm_frac" not in r["per_kernel"]["render_shade"]


def test_roofline_frame_block_and_hbm_entry_are_one_line_of_arithmetic(tmp_path, monkeypatch):
    """`roofline.frame` prices the step against the guide's two peaks from the committed counters -- every figure
    must be reproducible by hand: algorithmic bytes / step time / 8 TB/s (> 1, labelled), counter HBM bytes / step time / 8 TB/s,
    executed and useful MFMA flops / step time / 2.5 PFLOP/s, the rocprofv3 average beside the HIP-event time; counters of another
    WORKLOAD are refused like counters of another build; `roofline_hbm` carries the dense TV + Adam pass with the bytes it moved."""
    import json
    import bench
    code = bench.device_code_sha16()
    R, S, M = 2073600, 256, 26065245
    kern = {"render_march": 4.6, "render_shade": 4.0}
    pmc = {"device_code_sha16": code,
           "render_march": {"hbm_bytes": 5.7e9, "valu_insts": 3.64e9, "gui_active_cycles": 9.3e6, "rocprofv3_avg_ms": 4.7},
           "render_shade": {"hbm_bytes": 6.4e9, "valu_insts": 1.2e9, "mfma_busy_cycles": 3.5e9, "gui_active_cycles": 7.4e6, "rocprofv3_avg_ms": 4.1}}
    monkeypatch.setattr(bench, "PROFILE_DIR", str(tmp_path))
    (tmp_path / "pmc_summary.json").write_text(json.dumps(pmc))
    passes = M // 32
    r = bench.roofline_block(kern, M, R, S, passes, ms_per_step=8.7)
    fr = r["frame"]
    alg = R * S * 224 + R * 32 + M * 2688 + R * 24
    assert fr["algorithmic_bytes"] == alg and abs(fr["frac_of_hbm_algorithmic"] - alg / 8.7e-3 / 8e12) < 1e-9 and fr["frac_of_hbm_algorithmic"] > 2
    assert abs(fr["hbm_frac"] - 12.1e9 / 8.7e-3 / 8e12) < 1e-9 and "NOT a roofline fraction" in fr["frac_of_hbm_algorithmic_note"]
    assert abs(fr["mfma_executed_frac_of_2.5PF"] - passes * 132 * 32 * 32 * 16 * 2.0 / 8.7e-3 / 2.5e15) < 1e-9
    assert abs(fr["mfma_useful_frac_of_2.5PF"] - M * 43520.0 / 8.7e-3 / 2.5e15) < 1e-9 and fr["mfma_useful_frac_of_2.5PF"] < fr["mfma_executed_frac_of_2.5PF"]
    assert abs(fr["clock_GHz_profiled"]["render_march"] - 9.3e6 / 4.7e-3 / 1e9) < 1e-9
    pk = r["per_kernel"]["render_shade"]
    assert pk["rocprofv3_avg_ms"] == 4.1 and abs(pk["hip_event_over_rocprofv3"] - 4.0 / 4.1) < 1e-9
    # another workload (e.g. --freq 4): the S1 counters are refused, times and algorithmic rates stay
    r2 = bench.roofline_block(kern, M, R, S, passes, P=9, ms_per_step=8.7, pmc_workload_ok=False)
    assert "another workload" in r2["pmc_refused"] and r2["frame"]["hbm_bytes_pmc"] is None
    assert r2["frame"]["algorithmic_bytes"] == R * S * 288 + R * 32 + M * 3456 + R * 24
    # the HBM-bound kernel's entry
    tv = {"kernel": "ugrid_tv_adam_dense_cl", "ms": 4.3, "algorithmic_bytes": 24192000000, "achieved": 24192000000 / 4.3e-3 / 1e9}
    e = bench.hbm_roofline_entry(tv)
    assert e["bound"] == "hbm" and abs(e["frac"] - 24192000000 / 4.3e-3 / 8e12) < 1e-9 and e["traffic"] is None
    (tmp_path / "tv_adam_dense_pmc.json").write_text(json.dumps({"device_code_sha16": code, "hbm_bytes": 24.4e9, "hbm_read_bytes": 14.1e9, "hbm_write_bytes": 10.3e9}))
    e = bench.hbm_roofline_entry(tv)
    assert e["traffic"] == 24.4e9 and abs(e["traffic_over_algorithmic"] - 24.4e9 / 24192000000) < 1e-9
    (tmp_path / "tv_adam_dense_pmc.json").write_text(json.dumps({"device_code_sha16": "feedfeedfeedfeed", "hbm_bytes": 1.0}))
    assert bench.hbm_roofline_entry(tv)["traffic"] is None and "feedfeedfeedfeed" in bench.hbm_roofline_entry(tv)["pmc_refused"]


def test_tile_assignment_in_groups_partitions_the_rays():
    """dist.tile_assignment(group = K): every ray exactly once over the ranks for any ray count / world / group (ranks beyond the last
    group get none -- the world = 3 bug of round 5), consecutive tiles of a group stay together, rank 0 holds the largest share (the
    all-gather's padded tile size)"""
    from unboundednerfpytorch_amd.dist import tile_assignment
    for n in (0, 1, 63, 64, 65, 1000, 64 * 37 + 11, 64 * 240 * 3):
        for world in (1, 2, 3, 8):
            for group in (1, 4, 240):
                parts = [tile_assignment(n, world, r, group=group) for r in range(world)]
                allidx = torch.cat(parts) if parts else torch.empty(0)
                assert sorted(allidx.tolist()) == list(range(n)), (n, world, group)
                assert parts[0].numel() == max(p.numel() for p in parts)
                for p in parts:
                    if p.numel() > 1:
                        t = p // 64
                        jumps = (t[1:] - t[:-1])
                        assert bool(((jumps == 0) | (jumps == 1) | (jumps == (world - 1) * group + 1)).all()), (n, world, group)


def test_pixel_tile_order_is_a_permutation_and_untile_inverts_it():
    """fourier_render.pixel_tile_order / untile (8 x 8 pixel blocks per march wave): a permutation of the frame's pixels in
    which every run of 64 indices is one 8 x 8 block, inverted exactly by untile; None when H or W is not a multiple."""
    from unboundednerfpytorch_amd.fourier_render import pixel_tile_order, untile
    H, W = 24, 40
    order = pixel_tile_order(H, W, "cpu")
    assert order.dtype == torch.int64 and sorted(order.tolist()) == list(range(H * W))
    blk = order[64 * 7: 64 * 8]
    rows, cols = blk // W, blk % W
    assert int(rows.max() - rows.min()) == 7 and int(cols.max() - cols.min()) == 7           # one 8 x 8 block
    from unboundednerfpytorch_amd import fourier_render as fr
    if fr.TILE_MORTON:       # Z-order inside the block: every aligned run of 4 lanes is a 2 x 2 pixel quad, of 16 a 4 x 4 patch
        for q in range(0, 64, 4):
            assert int(rows[q:q + 4].max() - rows[q:q + 4].min()) == 1 and int(cols[q:q + 4].max() - cols[q:q + 4].min()) == 1
        for q in range(0, 64, 16):
            assert int(rows[q:q + 16].max() - rows[q:q + 16].min()) == 3 and int(cols[q:q + 16].max() - cols[q:q + 16].min()) == 3
    else:
        assert rows[:8].unique().numel() == 1 and cols[:8].tolist() == list(range(int(cols[0]), int(cols[0]) + 8))
    x = torch.arange(H * W * 3, dtype=torch.float32).view(H * W, 3)
    assert torch.equal(untile(x[order], H, W), x) and torch.equal(untile(x[order][:, 0].contiguous(), H, W), x[:, 0])
    assert pixel_tile_order(45, 77, "cpu") is None and pixel_tile_order(H, W, "cpu", tile=1) is None
    o4 = pixel_tile_order(H, W, "cpu", tile=4)
    assert torch.equal(untile(x[o4], H, W, tile=4), x)


def _sparse_exchange_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    torch.set_num_threads(1)
    from oracle import ref_ops
    from unboundednerfpytorch_amd.sharded_adam import ShardedMaskedAdam
    res = {}
    n_lines = 64 * world          # 64 lines per rank: n = 8192 floats, divisible by 64 * world
    for mode in ("masked", "dense_tv", "unmasked"):
        for sparse in (True, False):
            g = torch.Generator().manual_seed(7)
            p0 = torch.randn(n_lines * 64, generator=g).reshape(world, 4, 8, 8, 16)      # world x 64 lines
            p = torch.nn.Parameter(p0.clone())
            opt = ShardedMaskedAdam([{'params': [p], 'lr': 0.05, 'skip_zero_grad': mode != "unmasked"}], min_shard_numel=256, ops=ref_ops,
                                    sparse_exchange=sparse)
            ex = []
            for it in range(3):
                gg = torch.Generator().manual_seed(100 * it + rank)
                grad = torch.zeros(n_lines, 64)
                hit = torch.randperm(n_lines, generator=gg)[:6 + rank]          # a few lines per rank, different on each: with 8
                #                                                                 ranks some owners' ranges stay EMPTY in a step
                # values on a 2^-8 lattice: sums over <= 8 ranks are exact, so the packed and the dense reduce-scatter agree
                # whatever order the ring adds in (see _adam_case)
                vals = (torch.randn(hit.numel(), 64, generator=gg).clamp(-3.9, 3.9) * 256).round() / 256
                grad[hit] = vals * (torch.rand(hit.numel(), 64, generator=gg) > 0.3)
                p.grad = grad.reshape(p.shape).clone()
                tv = {p: (1e-3, mode == "dense_tv", None)} if mode != "unmasked" else None
                if tv is not None:
                    tv = {p: (1e-3, mode == "dense_tv", ref_ops)}
                opt.step(tv_terms=tv)
                ex.append(dict(opt.last_exchange[id(p)]))
            res[(mode, sparse)] = (p.detach().numpy().copy(), ex)
    q.put((rank, res))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", WORLDS)
def test_sparse_touched_line_exchange_equals_the_dense_collectives_gloo(world):
    """ShardedMaskedAdam exchanges the 256-byte lines some rank touched (bitmap all-gather + OR, packed
    reduce-scatter, packed all-gather of the updated rows) instead of the dense gradient / parameter ranges.  2, 3 and 8 gloo ranks
    (at 8, owners whose range nobody touched in a step), three update modes (masked TV + masked Adam; dense TV: sparse gradient
    exchange, dense parameter gather; plain Adam): the parameters after three steps equal the dense collectives' bit for bit on every
    rank, and the bytes on the wire shrink."""
    out = _spawn(_sparse_exchange_worker, world, 36100 + (os.getpid() + 17 * world) % 2000)
    for mode in ("masked", "dense_tv", "unmasked"):
        a0, ex_s = out[0][1][(mode, True)]
        d0, ex_d = out[0][1][(mode, False)]
        for r in range(1, world):
            assert np.array_equal(a0, out[r][1][(mode, True)][0]), (mode, r)      # every rank holds the same parameters
        assert np.array_equal(a0, d0), mode                     # = the dense collectives, bit for bit
        assert all(e["mode"] == "dense" for e in ex_d)
        for e in ex_s:
            assert e["reduce_scatter_bytes"] < e["dense_bytes_each_way"] // 3, e
            if mode == "masked":
                assert e["mode"] == "sparse" and e["all_gather_bytes"] < e["dense_bytes_each_way"] // 3, e
            else:                                               # every element of the range moves: the gather stays dense
                assert e["all_gather_bytes"] == e["dense_bytes_each_way"], e


def test_maybe_scale_grids_serves_both_model_families():
    """run_train.py:187-201: at a pg_scale step FourierGridModel.scale_volume_grid takes (density, rgb) voxel counts, DirectVoxGO /
    DirectContractedVoxGO one count -- which the reference's configs carry as `num_voxels_rgb`; the optimizer is rebuilt and
    act_shift lowered by decay_after_scale; any other step leaves everything alone"""
    import torch
    from unboundednerfpytorch_amd import train_step as ts

    class Stub(torch.nn.Module):
        def __init__(self, two):
            super().__init__()
            self.density = torch.nn.Linear(2, 2)
            self.register_buffer("act_shift", torch.zeros(1))
            self.calls = []
            if two:
                self.num_voxels_density = 1

        def scale_volume_grid(self, *a):
            self.calls.append(a)

    cfg_train = dict(pg_scale=[10, 20, 30], decay_after_scale=0.5, lrate_density=1e-1, lrate_decay=20, skip_zero_grad_fields=[])
    built = []
    orig = ts.create_optimizer_or_freeze_model
    ts.create_optimizer_or_freeze_model = lambda model, cfg, global_step, **kw: built.append(global_step) or "new-optimizer"
    try:
        for two, cfg_model, want in ((True, dict(num_voxels_density=8000, num_voxels_rgb=64000), [(2000, 16000), (4000, 32000), (8000, 64000)]),
                                     (False, dict(num_voxels_rgb=64000, num_voxels_density=1), [(16000,), (32000,), (64000,)]),
                                     (False, dict(num_voxels=64000), [(16000,), (32000,), (64000,)])):
            m = Stub(two)
            assert ts.maybe_scale_grids(m, "old", cfg_train, cfg_model, 11) == "old" and not m.calls
            for step in (10, 20, 30):
                assert ts.maybe_scale_grids(m, "old", cfg_train, cfg_model, step) == "new-optimizer"
            assert m.calls == want, (m.calls, want)
            assert float(m.act_shift) == -1.5
    finally:
        ts.create_optimizer_or_freeze_model = orig
    assert built == [0] * 9


def test_install_model_classes_rebinds_the_reference_classes(monkeypatch):
    """compat.install_model_classes: the reference's dvgo / dcvgo / FourierGrid_model modules then hand out this package's training
    models (same constructor arguments: built here with the reference's own keyword names), and the originals come back.  The
    function only rebinds attributes of the modules `FourierGrid.<name>` imports to, so those modules are stand-ins registered
    under the reference's names (each with its class, and run_train with its by-name import): nothing outside the repository."""
    import types
    from unboundednerfpytorch_amd import compat, fourier_model, voxgo_model
    pkg = types.ModuleType("FourierGrid")
    pkg.__path__ = []
    monkeypatch.setitem(sys.modules, "FourierGrid", pkg)
    mods = {}
    for name, cls in (("dvgo", "DirectVoxGO"), ("dcvgo", "DirectContractedVoxGO"), ("FourierGrid_model", "FourierGridModel")):
        m = types.ModuleType("FourierGrid." + name)
        setattr(m, cls, type(cls, (torch.nn.Module,), {}))
        setattr(pkg, name, m)
        monkeypatch.setitem(sys.modules, m.__name__, m)
        mods[name] = m
    dvgo, dcvgo, fgm = mods["dvgo"], mods["dcvgo"], mods["FourierGrid_model"]
    run_train = types.ModuleType("FourierGrid.run_train")
    run_train.FourierGridModel = fgm.FourierGridModel             # run_train.py:10 binds the class by name at import
    monkeypatch.setitem(sys.modules, run_train.__name__, run_train)
    orig = compat.install_model_classes()
    try:
        assert dvgo.DirectVoxGO is voxgo_model.DirectVoxGO and dcvgo.DirectContractedVoxGO is voxgo_model.DirectContractedVoxGO
        assert fgm.FourierGridModel is fourier_model.FourierGridModel and run_train.FourierGridModel is fourier_model.FourierGridModel
        # create_new_model's call shapes (run_train.py:32-50), incl. the extra keys its **model_kwargs carry
        extra = dict(num_voxels_base_density=8 ** 3, num_voxels_base_rgb=8 ** 3, num_voxels_viewdir=-1, density_type='DenseGrid',
                     k0_type='DenseGrid', density_config={}, k0_config={}, mpi_depth=128, nearest=False, pre_act_density=False,
                     in_act_density=False, bbox_thres=1e-3, mask_cache_thres=1e-3, rgbnet_dim=12, rgbnet_full_implicit=False,
                     rgbnet_direct=True, rgbnet_depth=3, rgbnet_width=128, alpha_init=1e-2, fast_color_thres=1e-4,
                     maskout_near_cam_vox=False, world_bound_scale=1.05, stepsize=0.5, fourier_freq_num=3, sample_num=-1)
        m1 = dvgo.DirectVoxGO(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=8 ** 3, num_voxels_base=extra['num_voxels_base_rgb'],
                              mask_cache_path=None, **extra)
        m2 = dcvgo.DirectContractedVoxGO(xyz_min=[-1, -1, -1], xyz_max=[1, 1, 1], num_voxels=8 ** 3, num_voxels_base=extra['num_voxels_base_rgb'],
                                         **extra)
        assert isinstance(m1, dvgo.DirectVoxGO) and isinstance(m2, dcvgo.DirectContractedVoxGO)
        assert set(m1.state_dict()) >= {"density.grid", "k0.grid", "mask_cache.mask", "rgbnet.0.weight"}
        assert m2.get_kwargs()["contracted_norm"] == "inf"
    finally:
        dvgo.DirectVoxGO, dcvgo.DirectContractedVoxGO, fgm.FourierGridModel = orig
    assert dvgo.DirectVoxGO is orig[0]


def test_fouriergrid_model_has_the_method_the_reference_program_calls():
    """run_train.py:160-161 calls model.gather_training_rays(...) for the FourierGrid datasets: the method delegates to train_rays"""
    from unboundednerfpytorch_amd import fourier_model, train_rays
    seen = {}
    orig = train_rays.gather_training_rays
    train_rays.gather_training_rays = lambda model, *a: seen.setdefault("args", (model,) + a) and "seven-tuple"
    try:
        m = fourier_model.FourierGridModel([-1, -1, -1], [1, 1, 1], num_voxels_density=8 ** 3, num_voxels_base_density=8 ** 3,
                                           num_voxels_rgb=8 ** 3, num_voxels_base_rgb=8 ** 3, alpha_init=1e-3, fourier_freq_num=1, rgbnet_dim=12)
        assert m.gather_training_rays("dd", "im", "cfg", "it", "ct", "po", "hw", "ks", "rk") == "seven-tuple"
        assert seen["args"] == (m, "dd", "im", "cfg", "it", "ct", "po", "hw", "ks", "rk")
    finally:
        train_rays.gather_training_rays = orig


def test_package_import_sets_the_hardware_queue_default_unless_given():
    """unboundednerfpytorch_amd/__init__.py: GPU_MAX_HW_QUEUES = 16 by setdefault (streams in flight need hardware queues of their own,
    profiles/r06/side_stream_queues.txt); an explicit setting of the caller's wins."""
    import subprocess
    code = "import os, unboundednerfpytorch_amd; print(os.environ['GPU_MAX_HW_QUEUES'])"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for given, want in ((None, "16"), ("4", "4")):
        env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
        if given is not None:
            env["GPU_MAX_HW_QUEUES"] = given
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == want, (out.stdout, out.stderr[-300:])
