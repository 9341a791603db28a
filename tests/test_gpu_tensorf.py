"""The TensoRF kernels (csrc/ugrid_tensorf.hip: query, query backward, total-variation gradient, bake) on the MI355X against the
float64 formula of tests/tensorf_cases.py, which the CPU suite ties to the reference's own float64 module (test_tensorf.py).

Bound, per tensor and point count: |HIP - fp64| <= 4 x the reference's recorded fp32-vs-fp64 error of that tensor on the same inputs
(tests/golden/tensorf_kernels.npz, written by gen_tensorf_golden.py), with a floor of half an ulp of the tensor's largest element under
the yardstick (see `check`); the last test prints the largest ratios measured.  Why 4: the kernels do the reference's fp32 operations in another
order (and the backward's atomics in a run-dependent one), which moves a maximum over the tensor by a small factor; a wrong corner,
weight, axis pairing or component count moves it by orders of magnitude.  Each test prints err / yardstick before it asserts."""
import functools
import os

import numpy as np
import pytest
import torch

import tensorf_cases as tc

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {c[0]: c for c in tc.KERNEL_CASES}
LAYOUTS = ("canonical", "complast")
SENTINEL = 12345.0
MARGIN = 64


@functools.lru_cache(maxsize=None)
def yards():
    return tc.load_yardsticks(GOLD)


@functools.lru_cache(maxsize=None)
def ref64(name, n):
    return tc.reference_f64(CASES[name], n)          # computed once per (case, n), shared by the tests, never modified


def stored(t, layout):
    t = t.cuda()
    return t.contiguous(memory_format=torch.channels_last) if (layout == "complast" and t.dim() == 4) else t.contiguous()


def device_inputs(name, layout):
    params, pts, grad_out = tc.case_inputs(CASES[name])
    p = {k: stored(torch.from_numpy(v), layout) for k, v in params.items()}
    lo, hi = torch.tensor(tc.XYZ_MIN).cuda(), torch.tensor(tc.XYZ_MAX).cuda()
    return p, torch.from_numpy(pts).cuda(), torch.from_numpy(grad_out).cuda(), lo, hi


RATIOS = {}          # (case, n, tensor) -> |hip - fp64| / effective yardstick, for the report of the last test of this file


def check(name, n, key, got, want):
    """|hip - fp64| <= 4 x max(yardstick of THIS point count, 2^-24 x the tensor's largest magnitude).
    The floor is half an ulp of the largest element, the rounding of ONE correctly rounded fp32 result: over one or a few elements
    (n = 1, a vector of two vertices) the reference's recorded maximum lies below it by chance -- at n = 1 its single forward value
    was 0.12 ulp off --, and no fp32 result in another operation order can be held to that.  Quantities that do not depend on the
    points (TV gradient, dense grid) are recorded once, under the full point count.  n = 0: exact zeros."""
    if n == 0:
        assert not np.asarray(got).any(), (name, n, key)
        return
    independent = key == 'dense' or key.startswith('tv_')
    err, scale = yards()[name]["n%d/%s" % (max(tc.N_POINTS) if independent else n, key)]
    eff = max(err, 2.0 ** -24 * scale)
    d = float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) if want.size else 0.0
    RATIOS[(name, n, key)] = max(RATIOS.get((name, n, key), 0.0), d / eff if eff else 0.0)
    print("%s n=%d %s: |hip - fp64| = %.3e, yardstick %.3e, floor %.3e (ratio %.2f), scale %.3e" % (name, n, key, d, err, 2.0 ** -24 * scale, d / eff if eff else 0.0, scale))
    assert np.isfinite(np.asarray(got)).all(), (name, n, key)
    assert d <= tc.BOUND_FACTOR * eff, (name, n, key, d, err, scale)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_query_forward(name, layout):
    from unboundednerfpytorch_amd import grid
    p, pts, _, lo, hi = device_inputs(name, layout)
    factors = tuple(p[k] for k in tc.FACTORS)
    for n in tc.N_POINTS:
        out = grid.tensorf_query(factors, p.get('f_vec'), pts[:n], lo, hi)
        assert tuple(out.shape) == ((n, CASES[name][5]) if 'f_vec' in p else (n,))
        check(name, n, 'out', out.cpu().numpy(), ref64(name, n)['out'])


def guarded_like(t):
    """a tensor of t's shape and strides inside a sentinel-filled buffer with MARGIN floats on both sides"""
    buf = torch.full((t.numel() + 2 * MARGIN,), SENTINEL, device=t.device)
    return buf, torch.as_strided(buf, t.shape, t.stride(), MARGIN)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_query_backward_all_seven_gradients_on_guarded_buffers(name, layout):
    from unboundednerfpytorch_amd import grid
    p, pts, go, lo, hi = device_inputs(name, layout)
    names = list(tc.FACTORS) + (['f_vec'] if 'f_vec' in p else [])
    factors = tuple(p[k] for k in tc.FACTORS)
    for n in tc.N_POINTS:
        bufs, views = zip(*[guarded_like(p[k]) for k in names])
        grads = list(views) + ([None] if 'f_vec' not in p else [])
        grid.tensorf_query_backward(go[:n], factors, p.get('f_vec'), pts[:n], lo, hi, grads=grads)
        torch.cuda.synchronize()
        for k, buf, v in zip(names, bufs, views):
            b = buf.cpu().numpy()
            assert (b[:MARGIN] == SENTINEL).all() and (b[-MARGIN:] == SENTINEL).all(), (name, n, k, "margin written")
            assert not (b[MARGIN:-MARGIN] == SENTINEL).any(), (name, n, k, "element not written")
            check(name, n, 'g_' + k, v.cpu().numpy(), ref64(name, n)['g_' + k])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_autograd_function_matches_and_gives_xyz_no_gradient(name, layout):
    from unboundednerfpytorch_amd import grid
    p, pts, go, lo, hi = device_inputs(name, layout)
    n = max(tc.N_POINTS)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    assert all(leaves[k].stride() == p[k].stride() for k in p)
    xyz = pts.clone().requires_grad_(True)
    out = grid.TensoRFQuery.apply(xyz, lo, hi, *[leaves[k] for k in tc.FACTORS], leaves.get('f_vec'))
    (out * go).sum().backward()
    assert xyz.grad is None
    for k, v in leaves.items():
        assert v.grad.stride() == v.stride()
        check(name, n, 'g_' + k, v.grad.cpu().numpy(), ref64(name, n)['g_' + k])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_tv_gradient_is_added_in_place(name, layout):
    from unboundednerfpytorch_amd import grid
    p, _, _, _, _ = device_inputs(name, layout)
    n = max(tc.N_POINTS)
    factors = tuple(p[k] for k in tc.FACTORS)
    grads = tuple(torch.zeros_like(t, memory_format=torch.preserve_format) for t in factors)
    grid.tensorf_tv_add_grad(factors, grads, *tc.TV_W)
    first = [g.clone() for g in grads]
    for k, g in zip(tc.FACTORS, grads):
        check(name, n, 'tv_' + k, g.cpu().numpy(), ref64(name, n)['tv_' + k])
    grid.tensorf_tv_add_grad(factors, grads, *tc.TV_W)            # added, not stored; gather form: the same bits every time
    for a, g in zip(first, grads):
        assert torch.equal(g, a + a)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(CASES))
def test_bake_both_output_layouts_and_dense_lookup(name, layout):
    from unboundednerfpytorch_amd import grid
    p, pts, _, lo, hi = device_inputs(name, layout)
    n = max(tc.N_POINTS)
    factors = tuple(p[k] for k in tc.FACTORS)
    want = ref64(name, n)
    baked = {}
    for cl in (False, True):
        d = grid.tensorf_bake(factors, p.get('f_vec'), channels_last=cl)
        assert tuple(d.shape) == want['dense'].shape
        if cl and d.shape[1] > 1:
            assert d.is_contiguous(memory_format=torch.channels_last_3d) and not d.is_contiguous()
        else:
            assert d.is_contiguous()
        check(name, n, 'dense', d.cpu().numpy(), want['dense'])
        baked[cl] = d
    assert torch.equal(baked[False], baked[True])
    # trilinear lookup of the baked grid = the factorised lookup (trilinear weights are separable): both under the forward's bound
    for cl in (False, True):
        q = grid.grid_query(baked[cl], pts, lo, hi, 0)
        check(name, n, 'out', q.cpu().numpy(), want['out'])
    check(name, n, 'out', grid.tensorf_query(factors, p.get('f_vec'), pts, lo, hi).cpu().numpy(), want['out'])


def test_module_adam_step_in_storage_layout():
    """MaskedAdam (skip-zero-grad kernels) on the component-last factors and f_vec: one step equals torch's Adam formula on the
    same gradients, element for element in the logical index space"""
    from unboundednerfpytorch_amd import grid
    from unboundednerfpytorch_amd.masked_adam import MaskedAdam
    torch.manual_seed(3)
    g = grid.TensoRFGrid(channels=3, world_size=torch.tensor([5, 7, 9]), xyz_min=tc.XYZ_MIN, xyz_max=tc.XYZ_MAX, config={'n_comp': 4, 'n_comp_xy': 2},
                         component_last=True).cuda()
    assert grid._lib.is_comp_last(g.xz_plane) and g.f_vec.is_contiguous()
    before = {k: v.detach().clone() for k, v in g.named_parameters()}
    opt = MaskedAdam([{'params': list(g.parameters()), 'lr': 0.1, 'skip_zero_grad': True}])
    pts = torch.from_numpy(tc.case_inputs(tc.KERNEL_CASES[0])[1]).cuda()
    g(pts).sum().backward()
    grads = {k: v.grad.detach().clone() for k, v in g.named_parameters()}
    opt.step()
    for k, v in g.named_parameters():
        gr = grads[k]
        # adam_upd_kernel.cu:60-75 at step 1, betas (0.9, 0.99): step size lr * sqrt(1 - b2) / (1 - b1), eps beside the uncorrected sqrt(v)
        m, s = 0.1 * gr, 0.01 * gr * gr
        step = (0.1 * (0.01 ** 0.5) / 0.1) * m / (s.sqrt() + 1e-8)
        want = torch.where(gr != 0, before[k] - step, before[k])
        assert v.stride() == before[k].stride()
        assert torch.allclose(v.detach(), want, rtol=1e-5, atol=1e-7), k


def test_zz_report_largest_ratios():
    """prints, per point count, the largest |hip - fp64| / yardstick the tests above measured (they assert <= 4)"""
    assert RATIOS, "runs after the kernel tests of this file"
    for n in tc.N_POINTS[1:]:
        worst = sorted(((r, k) for k, r in RATIOS.items() if k[1] == n), reverse=True)[:3]
        print("n=%d largest ratios: %s" % (n, ", ".join("%.2f %s %s" % (r, k[0], k[2]) for r, k in worst)))
