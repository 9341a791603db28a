"""Generate the DirectMPIGO fixtures (tests/golden/mpi_*.npz, rays_view_ndc.npz, mpi_ckpt_small.tar) by running the
REFERENCE's own Python model code (dmpigo.DirectMPIGO, dvgo.get_rays_of_a_view(ndc=True)) over the C oracle, like
gen_golden.py.  Runs only in the build container (needs the reference tree); inputs come from seeds (tests/mpi_cases.py).

    python tests/golden/gen_mpi_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = HERE
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mpi_cases  # noqa: E402
from oracle import install_stubs  # noqa: E402


def build_model(dmpigo, case):
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    model = dmpigo.DirectMPIGO(xyz_min=mpi_cases.XYZ_MIN, xyz_max=mpi_cases.XYZ_MAX, num_voxels=nvox, mpi_depth=D,
                               fast_color_thres=mpi_cases.fast_color_thres(stepsize, D), rgbnet_dim=C, rgbnet_depth=3,
                               rgbnet_width=mpi_cases.RGBNET_WIDTH, viewbase_pe=0)
    ws = [int(x) for x in model.world_size]
    assert ws == mpi_cases.world_size(nvox, D), ws
    sd = model.state_dict()
    params = mpi_cases.mpi_params(seed, ws, C, dm, ds)
    with torch.no_grad():
        for k, v in params.items():
            assert tuple(sd[k].shape) == tuple(v.shape), (k, sd[k].shape, v.shape)
            sd[k].copy_(torch.from_numpy(v))
    return model, ws


def gen_mpi():
    """dmpigo.DirectMPIGO.forward on NDC rays: the llff fine net (C = 9, width 64, viewbase_pe 0) and the no-rgbnet model."""
    dmpigo = install_stubs.import_reference("dmpigo")
    for case in mpi_cases.MPI_CASES:
        name, seed, D, nvox, C, stepsize, R, dm, ds = case
        model, ws = build_model(dmpigo, case)
        o, d, v = [torch.from_numpy(a) for a in mpi_cases.ndc_rays(seed, R)]
        with torch.no_grad():
            out = model(o, d, v, near=0, far=1, stepsize=stepsize, bg=1, render_depth=True)
        keep = {k: out[k].numpy() for k in ("alphainv_last", "weights", "rgb_marched", "raw_alpha", "raw_rgb", "ray_id", "depth")}
        keep["world_size"] = np.array(ws)
        keep["n_max"] = np.int64(out["n_max"])
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **keep)
        print(name, "world", ws, "N=%d" % out["n_max"], "M=%d" % out["weights"].numel(),
              "rgb mean %.3f" % float(out["rgb_marched"].mean()), "bg mean %.3f" % float(out["alphainv_last"].mean()))
        if name == "mpi_fine":
            ckpt = {"model_kwargs": model.get_kwargs(), "model_state_dict": model.state_dict()}
            torch.save(ckpt, os.path.join(OUT, "mpi_ckpt_small.tar"))


def gen_rays_view_ndc():
    """dvgo.get_rays_of_a_view(ndc=True) (dvgo.py:534-559) for a small forward-facing view and three flag combinations."""
    dvgo = install_stubs.import_reference("dvgo")
    K = np.array([[9.0, 0, 3.5], [0, 8.5, 2.5], [0, 0, 1]], dtype=np.float64)
    ang = 0.15
    c2w = np.array([[np.cos(ang), 0, np.sin(ang), 0.1], [0.02, 1.0, 0, -0.05], [-np.sin(ang), 0, np.cos(ang), 0.2]],
                   dtype=np.float32)
    res = {"K": K, "c2w": c2w}
    for tag, kw in (("a", dict(inverse_y=False, flip_x=False, flip_y=False)),
                    ("b", dict(inverse_y=True, flip_x=True, flip_y=False)),
                    ("c", dict(inverse_y=False, flip_x=False, flip_y=True))):
        o, d, v = dvgo.get_rays_of_a_view(H=6, W=8, K=K, c2w=torch.from_numpy(c2w), ndc=True, mode='center', **kw)
        res[tag + "_o"], res[tag + "_d"], res[tag + "_v"] = o.numpy(), d.numpy(), v.numpy()
    np.savez_compressed(os.path.join(OUT, "rays_view_ndc.npz"), **res)
    print("rays_view_ndc", o.shape, o.dtype)


if __name__ == "__main__":
    torch.set_num_threads(1)  # deterministic reduction order in F.linear / grid_sample
    gen_mpi()
    gen_rays_view_ndc()
