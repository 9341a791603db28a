"""Generate the TensoRF fixtures (tests/golden/tensorf_kernels.npz, tensorf_models.npz, tensorf_train.npz) by running the
REFERENCE's own Python code (grid.TensoRFGrid, dvgo.DirectVoxGO, dcvgo.DirectContractedVoxGO) over the oracle's stubs, like
gen_mpi_golden.py.  Runs only where the reference tree is; inputs come from seeds (tests/tensorf_cases.py).

    python tests/golden/gen_tensorf_golden.py [kernels] [models] [train]

Every quantity is computed twice, by the reference module as it is (float32) and by the same module after .double(); the
fixture keeps both and, per tensor, yard = (max |fp32 - fp64|, max |fp64|): the reference's own rounding error, the yardstick
of the GPU tests' bounds."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = HERE
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tensorf_cases as tc  # noqa: E402
from oracle import install_stubs  # noqa: E402


def yard(a32, a64):
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    if a64.size == 0:
        return np.array([0.0, 0.0])
    return np.array([np.abs(a32 - a64).max(), np.abs(a64).max()])


def ref_grid(grid_mod, case, dtype):
    name, seed, world, R, Rxy, C = case
    params, pts, grad_out = tc.case_inputs(case)
    cfg = {'n_comp': R}
    if Rxy != R:
        cfg['n_comp_xy'] = Rxy
    g = grid_mod.TensoRFGrid(channels=C, world_size=torch.tensor(world), xyz_min=tc.XYZ_MIN, xyz_max=tc.XYZ_MAX, config=cfg)
    sd = g.state_dict()
    with torch.no_grad():
        for k, v in params.items():
            assert tuple(sd[k].shape) == tuple(v.shape), (k, sd[k].shape, v.shape)
            sd[k].copy_(torch.from_numpy(v))
    return g.to(dtype), torch.from_numpy(pts).to(dtype), torch.from_numpy(grad_out).to(dtype)


def ref_values(grid_mod, case, n, dtype):
    """the reference module's forward on the first n points, the gradients of sum(out * grad_out), the TV gradient, the dense grid"""
    g, pts, go = ref_grid(grid_mod, case, dtype)
    names = [k for k, _ in g.named_parameters()]
    res = {}
    out = g(pts[:n])
    res['out'] = out.detach().numpy()
    if n > 0:
        (out * go[:n]).sum().backward()
    for k, p in g.named_parameters():
        res['g_' + k] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy()
        p.grad = None
    if n == max(tc.N_POINTS):
        g.total_variation_add_grad(*tc.TV_W, True)
        for k in tc.FACTORS:
            res['tv_' + k] = getattr(g, k).grad.detach().numpy().copy()
        with torch.no_grad():
            res['dense'] = g.get_dense_grid().numpy()
    return res, names


def gen_kernels():
    grid_mod = install_stubs.import_reference("grid")
    keep = {}
    for case in tc.KERNEL_CASES:
        name = case[0]
        worst = 0.0
        for n in tc.N_POINTS:
            r32, names = ref_values(grid_mod, case, n, torch.float32)
            r64, _ = ref_values(grid_mod, case, n, torch.float64)
            mine = tc.reference_f64(case, n)
            for k in r64:
                # the float64 formula of tensorf_cases.py is the reference in float64, to rounding
                d = np.abs(mine[k] - r64[k]).max() if r64[k].size else 0.0
                assert d <= 1e-12 * max(np.abs(r64[k]).max() if r64[k].size else 0.0, 1e-3), (name, n, k, d)
                keep["%s/n%d/%s/yard" % (name, n, k)] = yard(r32[k], r64[k])
                if n > 0 and r64[k].size and np.abs(r64[k]).max() > 0:
                    worst = max(worst, keep["%s/n%d/%s/yard" % (name, n, k)][0] / np.abs(r64[k]).max())
            if n == max(tc.N_POINTS):
                keep[name + "/out32"] = r32['out'][:tc.N_STORED].astype(np.float32)
                keep[name + "/out64"] = r64['out'][:tc.N_STORED]
                for k in r64:
                    if k.startswith(('g_', 'tv_')) and not name.startswith('path_'):
                        keep["%s/%s/32" % (name, k)] = r32[k].astype(np.float32)
                        keep["%s/%s/64" % (name, k)] = r64[k]
                keep[name + "/keys"] = np.array(names)
        print(name, "worst yardstick / scale %.2e" % worst)
    np.savez_compressed(os.path.join(OUT, "tensorf_kernels.npz"), **keep)
    print("tensorf_kernels.npz", os.path.getsize(os.path.join(OUT, "tensorf_kernels.npz")), "bytes")


class _Recorder:
    """wraps the reference's Alphas2Weights so that a forward leaves its pre-threshold weights behind"""
    def __init__(self, orig, log):
        self.orig, self.log = orig, log

    def apply(self, *a):
        out = self.orig.apply(*a)
        self.log.append(out[0].detach())
        return out


def ref_model(kind, kw):
    mod = install_stubs.import_reference("dvgo" if kind == "dvgo" else "dcvgo")
    return mod, (mod.DirectVoxGO if kind == "dvgo" else mod.DirectContractedVoxGO)(**kw)


def gen_models():
    """the reference's own DirectVoxGO / DirectContractedVoxGO with TensoRF grids on 64 rays: kept samples, per-sample and per-ray
    values, every parameter gradient of rgb_marched.sum(), in float32 and float64; no sample's alpha or weight within 1e-5 (relative)
    of fast_color_thres, so that the kept-sample list is the same in both precisions and can be demanded exactly"""
    keep = {}
    for name, kind, dtype_, seed, ray_seed in tc.MODEL_CASES:
        kw = tc.model_kwargs(kind, dtype_)
        torch.manual_seed(seed)
        mod, m = ref_model(kind, kw)
        tc.structure_density(m, dtype_)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        o, d, v = [torch.from_numpy(a) for a in tc.model_rays(64, ray_seed, kind)]
        rk = dict(tc.RENDER_KW) if kind == "dvgo" else dict(stepsize=0.5, bg=1)
        res = {}
        for prec in (torch.float32, torch.float64):
            torch.set_default_dtype(prec)
            try:
                m = m.to(prec)
                for p in m.parameters():
                    p.grad = None
                log, act = [], m.activate_density

                def recording(*a, _act=act, **k):
                    alpha = _act(*a, **k)
                    log.append(alpha.detach())
                    return alpha
                m.activate_density = recording
                orig, wlog = mod.Alphas2Weights, []
                mod.Alphas2Weights = _Recorder(orig, wlog)          # (the module-level name both forwards call)
                try:
                    out = m(o.to(prec), d.to(prec), v.to(prec), **rk)
                finally:
                    mod.Alphas2Weights = orig
                    del m.activate_density
                thres = kw['fast_color_thres']
                assert log and wlog, (name, len(log), len(wlog))
                for t in log + wlog:
                    assert float((t / thres - 1).abs().min()) > 1e-5, (name, "a sample sits on the threshold: choose another seed")
                out['rgb_marched'].sum().backward()
                res[prec] = ({k: out[k].detach().double().numpy() for k in tc.MODEL_KEYS + ('ray_id',)},
                             {k: p.grad.detach().double().numpy() for k, p in m.named_parameters()})
            finally:
                torch.set_default_dtype(torch.float32)
        (o32, g32), (o64, g64) = res[torch.float32], res[torch.float64]
        assert np.array_equal(o32['ray_id'], o64['ray_id']), name
        keep[name + "/ray_id"] = o32['ray_id'].astype(np.int64)
        for k in tc.MODEL_KEYS:
            keep["%s/out/%s/32" % (name, k)], keep["%s/out/%s/64" % (name, k)] = o32[k].astype(np.float32), o64[k]
        for k in g64:
            keep["%s/grad/%s/32" % (name, k)], keep["%s/grad/%s/64" % (name, k)] = g32[k].astype(np.float32), g64[k]
        for k, t in sd.items():
            keep["%s/sd/%s" % (name, k)] = t.numpy()
        print(name, "kept samples", len(o32['ray_id']), "rgb mean %.3f" % o64['rgb_marched'].mean(),
              "worst yardstick / scale %.2e" % max(yard(g32[k], g64[k])[0] / max(np.abs(g64[k]).max(), 1e-30) for k in g64))
    np.savez_compressed(os.path.join(OUT, "tensorf_models.npz"), **keep)
    print("tensorf_models.npz", os.path.getsize(os.path.join(OUT, "tensorf_models.npz")), "bytes")


def gen_train():
    """the reference's own 40 training steps (oracle/ref_train.run: the loop body of run_train.py:186-296 around the reference's model,
    optimizer and TV methods) of a TensoRF DirectVoxGO on the CPU, in float32 and in float64: the initial state and both final PSNRs"""
    from oracle import ref_train
    keep = {}
    kw = tc.model_kwargs("dvgo", "TensoRFGrid", width=128, nvox=tc.TRAIN_VOXELS // 2)
    o, d, v = [torch.from_numpy(a) for a in tc.model_rays(256, tc.TRAIN_RAY_SEED)]
    for prec in (torch.float32, torch.float64):
        torch.set_default_dtype(prec)
        try:
            torch.manual_seed(tc.TRAIN_SEED)
            _, m = ref_model("dvgo", kw)
            if prec == torch.float32:
                for k, t in m.state_dict().items():
                    keep["sd/" + k] = t.detach().clone().numpy()
            else:           # the same initial values as the float32 run, widened
                m.load_state_dict({k: torch.from_numpy(keep["sd/" + k]).to(prec if keep["sd/" + k].dtype.kind == "f" else None) for k in m.state_dict()})
            m = m.to(prec)
            batch = (o.to(prec), d.to(prec), v.to(prec), tc.train_target(v.to(prec)))
            hist = ref_train.run(m, "oracle", tc.TRAIN_CFG, dict(num_voxels=tc.TRAIN_VOXELS), [batch] * tc.TRAIN_STEPS, tc.TRAIN_STEPS, "cpu",
                                 render_kwargs=tc.RENDER_KW)
        finally:
            torch.set_default_dtype(torch.float32)
        tag = "32" if prec == torch.float32 else "64"
        keep["psnr/" + tag], keep["loss/" + tag] = np.array(hist["psnr_train"]), np.array(hist["loss"])
        print("train fp" + tag, "loss %.5f -> %.5f, psnr %.3f -> %.4f dB" % (hist["loss"][0], hist["loss"][-1], hist["psnr_train"][0], hist["psnr_train"][-1]))
    np.savez_compressed(os.path.join(OUT, "tensorf_train.npz"), **keep)
    print("tensorf_train.npz", os.path.getsize(os.path.join(OUT, "tensorf_train.npz")), "bytes")


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernels", "models", "train"]
    if "kernels" in what:
        gen_kernels()
    if "models" in what:
        gen_models()
    if "train" in what:
        gen_train()
