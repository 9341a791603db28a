"""Forward-facing DirectMPIGO path (dmpigo.DirectMPIGO, configs/llff): the composed forward of mpi_render.DirectMPIGORenderer
over the CPU oracle vs the reference's golden vectors, the state builders vs the checkpoint fixture, and the host NDC ray
chain vs the reference's get_rays_of_a_view(ndc=True).  No GPU needed."""
import os

import numpy as np
import pytest
import torch

import mpi_cases
from oracle import model_oracle, ref_ops


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=[c[0] for c in mpi_cases.MPI_CASES])
def test_mpi_oracle_matches_reference_golden(case, golden_dir):
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    gold = np.load(os.path.join(golden_dir, name + ".npz"))
    torch.set_num_threads(1)
    st = mpi_cases.state(case)
    assert st["world_size"].tolist() == gold["world_size"].tolist()
    rend = DirectMPIGORenderer(st, "cpu", ops=ref_ops, query=model_oracle.fourier_grid_query)
    assert not rend.fused_supported()
    o, d, v = [torch.from_numpy(a) for a in mpi_cases.ndc_rays(seed, R)]
    out = rend(o, d, v, near=0, far=1, stepsize=stepsize, bg=1, render_depth=True)
    assert out["n_max"] == int(gold["n_max"])
    assert np.array_equal(out["ray_id"].numpy(), gold["ray_id"])
    for k in ("alphainv_last", "weights", "rgb_marched", "raw_alpha", "raw_rgb", "depth"):
        np.testing.assert_allclose(out[k].numpy(), gold[k], rtol=2e-6, atol=2e-7, err_msg=k)


def test_mpi_act_shift_lerp_is_grid_sample():
    """the torch lerp of the [1,1,1,1,D] shift grid == grid_sample(align_corners=True), as the reference's DenseGrid evaluates
    it (grid.py: the one-voxel x / y axes), bit for bit, including points on the first / last plane"""
    import torch.nn.functional as F
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    st = mpi_cases.state(mpi_cases.MPI_CASES[0])
    rend = DirectMPIGORenderer(st, "cpu", ops=ref_ops, query=model_oracle.fourier_grid_query)
    lo, hi = st["xyz_min"], st["xyz_max"]
    u = torch.from_numpy(np.random.default_rng(3).random((4000, 3), dtype=np.float32))
    pts = lo + u * (hi - lo)
    pts[:5, 2] = lo[2]
    pts[5:10, 2] = hi[2]
    ind = ((pts - lo) / (hi - lo)).flip((-1,)) * 2 - 1
    ref = F.grid_sample(st["act_shift"], ind.reshape(1, 1, 1, -1, 3), mode='bilinear', align_corners=True).reshape(-1)
    assert torch.equal(rend.act_shift_at(pts), ref)


def test_mpi_state_builders_match_checkpoint(golden_dir):
    """mpi_state_from_params == mpi_state_from_reference_checkpoint(the reference's own checkpoint of the mpi_fine model), key by
    key; a TensoRF checkpoint raises"""
    from unboundednerfpytorch_amd.mpi_render import mpi_state_from_reference_checkpoint
    ref = mpi_cases.state(mpi_cases.MPI_CASES[0])
    ckpt = torch.load(os.path.join(golden_dir, "mpi_ckpt_small.tar"), map_location="cpu", weights_only=False)
    got = mpi_state_from_reference_checkpoint(ckpt)
    assert set(got) == set(ref)
    for k, v in ref.items():
        if torch.is_tensor(v):
            assert torch.equal(got[k], v), k
        elif isinstance(v, list):
            assert len(got[k]) == len(v) and all(torch.equal(a, b) for a, b in zip(got[k], v)), k
        else:
            assert got[k] == v, k
    assert got["voxel_size_ratio"] == ckpt["model_kwargs"]["voxel_size_ratio"]
    bad = {"model_kwargs": dict(ckpt["model_kwargs"], density_type="TensoRFGrid"), "model_state_dict": ckpt["model_state_dict"]}
    with pytest.raises(NotImplementedError, match="only DenseGrid checkpoints"):
        mpi_state_from_reference_checkpoint(bad)


def test_host_ndc_rays_match_reference(golden_dir):
    """fourier_render.get_rays_of_a_view(ndc=True) on host tensors == dvgo.get_rays_of_a_view(ndc=True); ndc=False unchanged"""
    from unboundednerfpytorch_amd.fourier_render import get_rays_of_a_view
    g = np.load(os.path.join(golden_dir, "rays_view_ndc.npz"))
    c2w = torch.from_numpy(g["c2w"])
    for tag, kw in (("a", dict(inverse_y=False, flip_x=False, flip_y=False)),
                    ("b", dict(inverse_y=True, flip_x=True, flip_y=False)),
                    ("c", dict(inverse_y=False, flip_x=False, flip_y=True))):
        o, d, v = get_rays_of_a_view(6, 8, g["K"], c2w, ndc=True, **kw)
        for a, k in ((o, "_o"), (d, "_d"), (v, "_v")):
            np.testing.assert_allclose(a.numpy(), g[tag + k], rtol=1e-6, atol=1e-7, err_msg=tag + k)
        o2, d2, v2 = get_rays_of_a_view(6, 8, g["K"], c2w, **kw)
        assert torch.equal(v2, v) and not torch.equal(o2, o)
