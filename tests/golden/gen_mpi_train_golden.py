"""Generate the DirectMPIGO TRAINING fixtures (tests/golden/mpi_train_<case>.npz, mpi_train_rays.npz) by running the REFERENCE's
own Python code (dmpigo.DirectMPIGO, dvgo.get_training_rays / get_training_rays_flatten with ndc=True) over the C oracle on the
CPU, like gen_mpi_golden.py and gen_golden.gen_voxgo_train.  Runs only in the build container (needs the reference tree);
inputs come from seeds (tests/mpi_cases.py).

    python tests/golden/gen_mpi_train_golden.py
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
sys.path.insert(0, HERE)

import mpi_cases  # noqa: E402
import synth  # noqa: E402
from gen_mpi_golden import build_model  # noqa: E402
from oracle import install_stubs  # noqa: E402

SCALED_K0_CHANNELS = [0, 4, 8]
MIN_KEPT = 500      # fewer surviving samples and the per-sample / gradient comparisons of tests/test_gpu_mpi_train.py mean little


def golden_loss(out, target, R):
    """test_gpu_voxgo_train.golden_loss' terms: MSE + 0.01 entropy_last (run_train.py:254-261) + 0.05 sum w^2 / R"""
    loss = torch.nn.functional.mse_loss(out["rgb_marched"], target)
    pout = out["alphainv_last"].clamp(1e-6, 1 - 1e-6)
    loss = loss + 0.01 * (-(pout * torch.log(pout) + (1 - pout) * torch.log(1 - pout))).mean()
    return loss + 0.05 * (out["weights"] * out["weights"]).sum() / R


def ray_scene():
    """three tiny forward-facing views: (imgs [3,H,W,3], poses [3,3,4], HW, Ks) -- equal sizes, so both table functions apply"""
    H, W = 5, 7
    K = np.array([[9.0, 0, 3.5], [0, 8.5, 2.5], [0, 0, 1]], dtype=np.float64)
    poses = []
    for ang, t in ((0.15, (0.1, -0.05, 0.2)), (-0.1, (-0.2, 0.1, 0.15)), (0.02, (0.0, 0.0, 0.3))):
        poses.append([[np.cos(ang), 0, np.sin(ang), t[0]], [0.02, 1.0, 0, t[1]], [-np.sin(ang), 0, np.cos(ang), t[2]]])
    poses = torch.tensor(np.array(poses, dtype=np.float32))
    imgs = torch.from_numpy(synth.uniform(77, 3 * H * W * 3).reshape(3, H, W, 3).astype(np.float32))
    return imgs, poses, np.array([[H, W]] * 3), np.stack([K] * 3)


def gen_mpi_train():
    dmpigo = install_stubs.import_reference("dmpigo")
    for case in mpi_cases.MPI_CASES:
        name, seed, D, nvox, C, stepsize, R, dm, ds = case
        fresh = dmpigo.DirectMPIGO(xyz_min=mpi_cases.XYZ_MIN, xyz_max=mpi_cases.XYZ_MAX, num_voxels=nvox, mpi_depth=D,
                                   fast_color_thres=mpi_cases.fast_color_thres(stepsize, D), rgbnet_dim=C, rgbnet_depth=3,
                                   rgbnet_width=mpi_cases.RGBNET_WIDTH, viewbase_pe=0)
        res = {"fresh_act_shift": fresh.act_shift.grid.detach().numpy().copy()}
        model, ws = build_model(dmpigo, case)
        o, d, v = [torch.from_numpy(a) for a in mpi_cases.ndc_rays(seed, R)]
        kw = dict(near=0, far=1, stepsize=stepsize, bg=1, render_depth=True)
        target = torch.from_numpy(synth.uniform(seed + 5, R * 3).reshape(R, 3).astype(np.float32))
        out = model(o, d, v, global_step=1, **kw)
        loss = golden_loss(out, target, R)
        loss.backward()
        res.update({"loss": loss.detach().numpy(), "n_kept": np.int64(out["weights"].numel()), "target": target.numpy(),
                    "n_max": np.int64(out["n_max"]), "world_size": np.array(ws), "ratio": np.float32(model.voxel_size_ratio)})
        for k in ("rgb_marched", "alphainv_last", "weights", "ray_id", "raw_rgb", "raw_alpha", "depth", "s"):
            res[k] = out[k].detach().numpy()
        for k, p in model.named_parameters():
            if p.grad is not None:
                res["grad." + k] = p.grad.numpy().copy()
        sd = model.state_dict()
        res["sd_keys"] = np.array(sorted(sd.keys()))
        res["sd_shapes"] = np.array([str(tuple(sd[k].shape)) for k in sorted(sd.keys())])
        res["kwargs_keys"] = np.array(sorted(model.get_kwargs().keys()))
        model.zero_grad()
        model.update_occupancy_cache()
        res["occ_mask"] = model.mask_cache.mask.numpy().copy()
        model.scale_volume_grid(2 * nvox, D)
        res["scaled_density"] = model.density.grid.detach().numpy().copy()
        # (every channel is resampled alone: three of the nine in fp32 and the others rounded to fp16 keep the fine case's file under
        # the size limit of a committed file)
        res["scaled_k0_channels"] = np.array(SCALED_K0_CHANNELS if C > 3 else list(range(3)))
        k0s = model.k0.grid.detach().numpy()
        res["scaled_k0"] = k0s[:, res["scaled_k0_channels"]].copy()
        rest = [c for c in range(k0s.shape[1]) if c not in res["scaled_k0_channels"].tolist()]
        res["scaled_k0_rest_channels"] = np.array(rest, dtype=np.int64)
        res["scaled_k0_rest_f16"] = k0s[:, rest].astype(np.float16)
        res["scaled_mask"] = model.mask_cache.mask.numpy().copy()
        res["scaled_world_size"] = model.world_size.numpy().copy()
        with torch.no_grad():
            out2 = model(o, d, v, global_step=2, **kw)
        res["scaled_rgb_marched"] = out2["rgb_marched"].numpy()
        res["scaled_n_kept"] = np.int64(out2["weights"].numel())
        path = os.path.join(OUT, "mpi_train_" + name + ".npz")
        np.savez_compressed(path, **res)
        print("mpi_train", name, "world", ws, "N=%d" % out["n_max"], "loss %.6f kept %d; occupancy %d / %d; scaled to %s kept %d; %d bytes" % (
            float(loss), int(res["n_kept"]), int(res["occ_mask"].sum()), res["occ_mask"].size, res["scaled_world_size"].tolist(),
            int(res["scaled_n_kept"]), os.path.getsize(path)))
        assert int(res["n_kept"]) >= MIN_KEPT, (name, int(res["n_kept"]))


def gen_ndc_ray_tables():
    """dvgo.get_training_rays(ndc=True) (dvgo.py:562-590) and get_training_rays_flatten(ndc=True) (:594-616) of three tiny views"""
    dvgo = install_stubs.import_reference("dvgo")
    imgs, poses, HW, Ks = ray_scene()
    flags = dict(inverse_y=False, flip_x=False, flip_y=True)
    res = {}
    r = dvgo.get_training_rays(rgb_tr=imgs, train_poses=poses, HW=HW, Ks=Ks, ndc=True, **flags)
    for k, t in zip(("rgb", "o", "d", "v"), r[:4]):
        res["img_" + k] = t.numpy()
    res["img_imsz"] = np.array(r[4])
    r = dvgo.get_training_rays_flatten(rgb_tr_ori=list(imgs), train_poses=poses, HW=HW, Ks=Ks, ndc=True, **flags)
    for k, t in zip(("rgb", "o", "d", "v"), r[:4]):
        res["flat_" + k] = t.numpy()
    res["flat_imsz"] = np.array(r[4])
    np.savez_compressed(os.path.join(OUT, "mpi_train_rays.npz"), **res)
    print("mpi_train_rays", res["img_o"].shape, res["flat_o"].shape)


if __name__ == "__main__":
    torch.set_num_threads(1)  # deterministic reduction order in F.linear / grid_sample
    gen_mpi_train()
    gen_ndc_ray_tables()
