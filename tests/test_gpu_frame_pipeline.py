"""dist.FramePipeline and run_render.render_viewpoints over a process group, on the real kernels: worker processes as
tests/test_gpu_multi.py starts them (a fresh process per rank, gloo, the ranks share the GPU present), one launch per world size.
Every rank's assembled frames must equal the single-process render_view of the same renderer BITWISE: a ray's result is formed by its
own lane in the march and shade kernels, so neither the split nor the ray order of a rank's share can show."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RENDERERS = ("fourier", "dvgo", "dcvgo", "mpi")

# the renderers at the smallest shapes of their own GPU tests (test_gpu_multi.py, test_dvgo.py, test_dcvgo.py, test_gpu_mpi.py)
COMMON = r'''
import numpy as np
import torch
import mpi_cases
from test_oracle_golden import make_state


def make_renderer(name, dev):
    if name == "fourier":
        from unboundednerfpytorch_amd.fourier_render import FourierGridRenderer
        return FourierGridRenderer(make_state(seed=5, G=24, F=3, C=12, pe=4, norm="inf", thres=1e-4, dm=6.0, ds=12.0), dev), dict(stepsize=0.5)
    if name == "dvgo":
        from test_dvgo import dvgo_state
        from unboundednerfpytorch_amd.dvgo_render import DirectVoxGORenderer
        state, _ = dvgo_state(79, 48, 12, True, 1.0, 4.0, [-0.67, -1.2, -0.37], [0.67, 1.2, 1.03])
        return DirectVoxGORenderer(state, dev), dict(near=2.0, far=6.0, stepsize=0.5, bg=1)
    if name == "dcvgo":
        from test_dcvgo import dcvgo_state
        from unboundednerfpytorch_amd.dcvgo_render import DirectContractedVoxGORenderer
        state, _ = dcvgo_state(81, 40, 40, 12, "inf", 2.0, 6.0)
        return DirectContractedVoxGORenderer(state, dev), dict(stepsize=0.5, bg=torch.tensor([0.2, 0.5, 0.9], device=dev))
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    case = mpi_cases.MPI_CASES[0]
    return DirectMPIGORenderer(mpi_cases.state(case), dev), dict(near=0, far=1, stepsize=case[5], bg=1)


def views(name, sizes=((16, 24), (13, 7), (16, 24))):
    """three views with different poses; the second has another frame size: 16 x 24 takes block order, 13 x 7 image order"""
    out = []
    for i, (H, W) in enumerate(sizes):
        f = 60.0 if name == "dvgo" else 30.0
        K = [[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]
        if name == "dvgo":
            c2w = [[-0.9999, 0.0042, -0.0133, -0.0538 + 0.03 * i], [-0.0140, -0.2997, 0.9539, 3.8455], [0.0, 0.9540, 0.2997, 1.2081 + 0.01 * i]]
        elif name == "mpi":
            a = 0.04 * i - 0.05
            c2w = [[np.cos(a), 0, np.sin(a), 0.1 * a], [0, 1, 0, 0.02], [-np.sin(a), 0, np.cos(a), 0.05]]
        else:
            c2w = [[1.0, 0, 0, 0.1 + 0.05 * i], [0, 0.8, 0.6, -0.2], [0, -0.6, 0.8, 0.3 + 0.04 * i]]
        out.append((H, W, K, torch.tensor(c2w, dtype=torch.float32)))
    return out


def render_view_packed(name, rend, kw, H, W, K, c2w):
    """the single-process frame: the renderer's own render_view, packed [H*W,5]"""
    if name == "fourier":
        rgb, depth, last = rend.render_view(H, W, K, c2w, kw["stepsize"])
    else:
        out = rend.render_view(H, W, K, c2w, render_depth=True, **kw)
        rgb, depth, last = out["rgb_marched"], out["depth"], out["alphainv_last"]
    return torch.cat([rgb.reshape(-1, 3), depth.reshape(-1, 1), last.reshape(-1, 1)], dim=1)


def viewpoints_case(dev):
    """render_viewpoints' arguments for a three-view list with ground truth (one frame size: the function returns stacked arrays)"""
    rend, kw = make_renderer("dvgo", dev)
    vs = views("dvgo", ((16, 24),) * 3)
    HW, Ks, poses = [(v[0], v[1]) for v in vs], [v[2] for v in vs], [v[3].numpy() for v in vs]
    rs = np.random.RandomState(7)
    gt = [rs.uniform(0, 1, (H, W, 3)).astype(np.float32) for H, W in HW]
    return rend, poses, HW, Ks, kw, gt
'''

WORKER = COMMON + r'''
import json, os, sys
import torch.distributed as dist
ROOT = sys.argv[1]; what = sys.argv[2]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
local = int(os.environ["LOCAL_RANK"]) % torch.cuda.device_count()
torch.cuda.set_device(local)
dev = torch.device("cuda", local)
dist.init_process_group("gloo", rank=rank, world_size=world)
from unboundednerfpytorch_amd.dist import FramePipeline
res = {}
if what == "viewpoints":
    from unboundednerfpytorch_amd.run_render import render_viewpoints
    rend, poses, HW, Ks, kw, gt = viewpoints_case(dev)
    got = render_viewpoints(rend, poses, HW, Ks, kw, gt_imgs=gt, eval_ssim=True, deal="tiles")
    np.savez(os.path.join(sys.argv[3], "viewpoints_rank%d.npz" % rank), psnrs=np.array(got[3]), ssims=np.array(got[4]),
             **{"a%d_%d" % (j, i): got[j][i] for j in range(3) for i in range(len(poses))})
    res["done"] = True
else:
    for name in what.split(","):
        rend, kw = make_renderer(name, dev)
        vs = views(name)
        want = [render_view_packed(name, rend, kw, *v) for v in vs]
        for deal in ("bands", "tiles"):
            pipe = FramePipeline(rend, deal=deal)
            got = [pipe.submit(*v, **kw) for v in vs] + [pipe.flush()]
            ok = got[0] is None and pipe.world == world
            ok = ok and all(g is not None and g.shape == w.shape and torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got[1:], want))
            # (a frame that is all background would make the comparison empty)
            covered = min(float((w[:, 4] < 0.99).float().mean()) for w in want[::2])
            res["%s/%s" % (name, deal)] = {"bitwise": bool(ok), "covered": covered, "distinct": not torch.equal(want[0], want[2])}
torch.cuda.synchronize()
allres = [None] * world
dist.all_gather_object(allres, res)
if rank == 0:
    print("RESULT " + json.dumps(allres))
dist.destroy_process_group()
'''


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


@functools.lru_cache(maxsize=None)
def _run(what, world, outdir=""):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "frame_pipeline_worker.py")          # torch.distributed.run wants a script file
        with open(path, "w") as f:
            f.write(WORKER)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), path, ROOT, what, outdir]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


@pytest.mark.parametrize("deal", ["bands", "tiles"])
@pytest.mark.parametrize("name", RENDERERS)
@pytest.mark.parametrize("world", [2, 3])
def test_every_renderer_sharded_is_bitwise_its_single_process_render_view(world, name, deal):
    res = _run(",".join(RENDERERS), world)          # (one launch per world size, shared by the cases)
    assert len(res) == world
    for r in res:
        c = r["%s/%s" % (name, deal)]
        assert c["bitwise"] is True and c["distinct"] is True and c["covered"] > 0.05, c


@pytest.mark.parametrize("deal", ["bands", "tiles"])
def test_fourier_renderer_at_world_8(deal):
    """8 ranks over 6 tiles (16 x 24) and 2 tiles (13 x 7): ranks without rays send zero tiles and assemble every frame"""
    res = _run("fourier", 8)
    assert len(res) == 8
    for r in res:
        assert r["fourier/" + deal]["bitwise"] is True


def _common():
    ns = {}
    exec(compile(COMMON, "frame_pipeline_common", "exec"), ns)
    return ns


def test_render_viewpoints_over_two_ranks_returns_the_single_process_arrays_and_scores(tmp_path):
    from unboundednerfpytorch_amd.run_render import render_viewpoints
    res = _run("viewpoints", 2, str(tmp_path))
    assert [r["done"] for r in res] == [True, True]
    rend, poses, HW, Ks, kw, gt = _common()["viewpoints_case"](torch.device("cuda:0"))
    want = render_viewpoints(rend, poses, HW, Ks, kw, gt_imgs=gt, eval_ssim=True)
    for rank in range(2):
        got = np.load(os.path.join(str(tmp_path), "viewpoints_rank%d.npz" % rank))
        for j in range(3):
            for i in range(3):
                assert np.array_equal(got["a%d_%d" % (j, i)].view(np.int32), want[j][i].view(np.int32)), (rank, j, i)
        assert np.array_equal(got["psnrs"], np.array(want[3])) and np.array_equal(got["ssims"], np.array(want[4]))
    assert float(want[2].mean()) < 0.99 and not np.array_equal(want[0][0], want[0][2])


@pytest.mark.parametrize("name", RENDERERS)
def test_fused_assembly_on_and_off_return_identical_arrays(name):
    from unboundednerfpytorch_amd import run_render
    ns = _common()
    rend, kw = ns["make_renderer"](name, torch.device("cuda:0"))
    saved = run_render.FUSED_ASSEMBLY
    for H, W in ((16, 24), (13, 7)):                # block order / image order (one size per call: the arrays come back stacked)
        vs = ns["views"](name, ((H, W),) * 3)
        args = (rend, [v[3].numpy() for v in vs], [(H, W)] * 3, [v[2] for v in vs], kw)
        try:
            run_render.FUSED_ASSEMBLY = True
            on = run_render.render_viewpoints(*args)
            run_render.FUSED_ASSEMBLY = False
            off = run_render.render_viewpoints(*args)
        finally:
            run_render.FUSED_ASSEMBLY = saved
        for a, b in zip(on, off):
            assert a.shape[:3] == (3, H, W) and np.array_equal(a.view(np.int32), b.view(np.int32))
        # ... and they are the renderer's own render_view
        w = ns["render_view_packed"](name, rend, kw, *vs[1]).cpu().numpy().reshape(H, W, 5)
        assert np.array_equal(on[0][1], w[..., 0:3]) and np.array_equal(on[1][1], w[..., 3:4]) and np.array_equal(on[2][1], w[..., 4:5])
        assert not np.array_equal(on[0][0], on[0][1])
