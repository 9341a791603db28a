"""CPU checks of tests/march_cases.py, the harness of tests/test_gpu_march_worklist.py: its float32 reference against the pinned
oracles (so the float64 one is the same formula), and the conditions under which no GPU test hides a failure -- the margin of every
case, the share of rays set aside, the presence and decidability of every named edge, the e32 limits.

Measured here (all 72 cases, this file's own output with -s):
  margin m = K * the widest float32-vs-float64 error of a thresholded quantity: 0 .. 9.2e-5, within M_LIMIT = 1e-4 on every case
  (largest: the T < 1e-3 decision behind an opaque sample, T = 3e-5 +- 1.2e-8).  It holds because the densities are chosen for it:
  alpha = 1 - (1 + exp(x)) ^ -interval carries 2^-24 of ABSOLUTE rounding, 6e-4 of a threshold of 1e-4, so no scene here has a
  sample whose alpha lies between 1e-9 and 0.01 (march_cases.density_field: `surfaces` is two-valued, EMPTY = -3e6 | alpha 0.85).
  share of rays set aside: at most 0.5 % (one ray of dcvgo's shell case, on the cumdist threshold).
  e32: w 6.9e-7, alphainv_last 6.9e-7, depth 1.1e-6, wsum_mid 2.4e-7, positions 1.35e-7 of the extent."""
import numpy as np
import pytest
import torch

import march_cases as mc
import mpi_cases
import shade_cases
import synth
from oracle import model_oracle, ref_ops
from test_oracle_golden import FG_CASES, make_state

ALL = mc.all_cases()
IDS = [c.name for c in ALL]


def _close(a, b, what):
    # within rounding: the oracle's own 2e-6 relative (tests/test_oracle_golden.py), and absolutely one ulp of 1.0 -- alpha = 1 - pow
    # is rounded on that grid, and grid_sample's vector body and scalar tail differ by an ulp according to where a point stands in
    # the batch ([R, S] points here, the compacted list in the oracle), which moves a transmittance of 6e-4 by 4e-9
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=2e-6, atol=2.0 ** -23, err_msg=what)


def _pin(ref, out, R, keys=("alphainv_last", "depth"), step_id=True):
    """index arrays exact, floats within rounding: the float32 reference run against an oracle forward's outputs"""
    ray_id, sid, w = mc.survivors(ref)
    assert torch.equal(ray_id, out["ray_id"].long())
    if step_id:
        assert torch.equal(sid, out["step_id"].long())
    _close(w, out["weights"], "weights")
    _close(ref.last, out["alphainv_last"], "alphainv_last")
    _close(ref.depth, out["depth"], "depth")
    if "wsum_mid" in keys:
        _close(ref.wsum_mid, out["wsum_mid"], "wsum_mid")


# ---------------------------------------------------------------------------------------------------------------------
# the float32 reference against the pinned oracles
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FG_CASES, ids=[c[0] for c in FG_CASES])
def test_fourier_reference_is_the_pinned_oracle(case):
    name, seed, G, F, C, pe, norm, stepsize, R, thres, dm, ds = case
    torch.set_num_threads(1)
    state = make_state(seed, G, F, C, pe, norm, thres, dm, ds)
    o, d, v = [torch.from_numpy(a) for a in synth.rays(seed, R)]
    out = model_oracle.fouriergrid_render(state, o, d, v, stepsize, render_depth=True)
    ref = mc.march_reference(state, o, d, stepsize, torch.float32)
    assert ref.h.S == out["n_max"] and int(ref.surv.sum()) > R
    _pin(ref, out, R)


def test_dvgo_reference_is_the_pinned_oracle():
    from test_dvgo import DVGO_CASES, dvgo_state
    from unboundednerfpytorch_amd.dvgo_render import DirectVoxGORenderer
    torch.set_num_threads(1)
    for name, seed, G, C, direct, R, dm, ds in DVGO_CASES:
        state, _ = dvgo_state(seed, G, C, direct, dm, ds)
        o, d, v = [torch.from_numpy(a) for a in synth.rays(seed, R, origin_scale=0.4)]
        out = model_oracle.dvgo_render(state, o, d, v, 0.2, 0.5, 1, ref_ops, model_oracle.fourier_grid_query)
        fused = DirectVoxGORenderer(state, "cpu", ops=ref_ops, query=model_oracle.fourier_grid_query)._fused_state()
        ref = mc.march_reference(fused, o, d, 0.5, torch.float32, near=0.2)
        assert int(ref.n.max()) <= ref.h.S and int(ref.surv.sum()) > R // 2
        _pin(ref, out, R, step_id=False)


@pytest.mark.parametrize("case", synth.DCVGO_CASES, ids=[c[0] for c in synth.DCVGO_CASES])
def test_dcvgo_reference_is_the_pinned_composition(case):
    from test_dcvgo import dcvgo_rays, dcvgo_state
    from unboundednerfpytorch_amd.dcvgo_render import DirectContractedVoxGORenderer
    name, seed, G, Gb, C, norm, R, dm, ds = case
    torch.set_num_threads(1)
    state, _ = dcvgo_state(seed, G, Gb, C, norm, dm, ds)
    o, d, v = dcvgo_rays(seed, R)
    rend = DirectContractedVoxGORenderer(state, "cpu", ops=ref_ops, query=model_oracle.fourier_grid_query)
    out = rend(o, d, v, stepsize=0.5, bg=1, render_depth=True)
    ref = mc.march_reference(rend._fused_state(), o, d, 0.5, torch.float32)
    assert ref.h.S == out["n_max"] and int(ref.surv.sum()) > 0
    _pin(ref, out, R, keys=("alphainv_last", "depth", "wsum_mid"))


@pytest.mark.parametrize("case", mpi_cases.MPI_CASES, ids=[c[0] for c in mpi_cases.MPI_CASES])
def test_mpi_reference_is_the_pinned_composition(case):
    from unboundednerfpytorch_amd.mpi_render import DirectMPIGORenderer
    name, seed, D, nvox, C, stepsize, R, dm, ds = case
    torch.set_num_threads(1)
    rend = DirectMPIGORenderer(mpi_cases.state(case), "cpu", ops=ref_ops, query=model_oracle.fourier_grid_query)
    o, d, v = [torch.from_numpy(a) for a in mpi_cases.ndc_rays(seed, R)]
    out = rend(o, d, v, near=0, far=1, stepsize=stepsize, bg=1, render_depth=True)
    ref = mc.march_reference(rend._fused_state(), o, d, stepsize, torch.float32)
    assert ref.h.S == out["n_max"] and int(ref.surv.sum()) > 0
    _pin(ref, out, R, step_id=False)


def test_float64_reference_is_the_same_formula():
    """the float64 run of a case differs from its float32 run by rounding only: same decisions on all but the rays set aside"""
    for c in ALL[:6]:
        a = mc.analysis(c)
        assert float(a.same32.float().mean()) >= 1 - mc.SET_ASIDE_LIMIT, c.name


# ---------------------------------------------------------------------------------------------------------------------
# the conditions under which no GPU test hides a failure
# ---------------------------------------------------------------------------------------------------------------------
def test_layout_is_shade_cases_own():
    assert mc.worklist_regions is shade_cases.worklist_regions and mc.read_worklist is shade_cases.read_worklist
    assert len(set(IDS)) == len(IDS)
    assert sorted({c.R for c in ALL}) == sorted(mc.RAY_COUNTS)
    assert all(c.S <= 48 for c in ALL)
    nt = (mc.RAY_COUNTS[3] + 63) // 64
    assert nt == 37 and (nt + 3) // 4 == 10                       # 10 blocks in a grid of 16: the XCD remap skips six
    assert (mc.RAY_COUNTS[2] + 63) // 64 == 6 and mc.RAY_COUNTS[1] % 64 == 8


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_margin_of_every_case(case):
    a = mc.analysis(case)
    print("march-margin %s: m = %.3g  %s" % (case.name, a.m, {k: "%.2g" % v for k, v in a.m_dec.items()}))
    assert a.m <= mc.M_LIMIT


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_share_set_aside_and_e32(case):
    a = mc.analysis(case)
    print("march-case %s: m = %.3g, set aside %.3f, e32 %s" % (case.name, a.m, a.set_aside, {k: "%.2g" % v for k, v in a.e32.items()}))
    assert a.set_aside <= mc.SET_ASIDE_LIMIT
    for k, v in a.e32.items():
        assert v <= mc.E32_LIMIT[k], (k, v)
    assert a.bound("w") <= 1e-5 and a.bound("pos") <= 4e-6           # no bound is loose: a tenth of the frames' 1e-4 and of the weight threshold
    r = a.r64                                                        # neighbouring steps lie far further apart than the position bound
    if case.S > 1:
        gap = (r.pos[:, 1:] - r.pos[:, :-1]).abs().amax(-1)
        both = r.ran[:, 1:] & r.ran[:, :-1]
        if bool(both.any()):
            assert float(gap[both].min()) > 100 * a.bound("pos"), float(gap[both].min())


def _tiles(R):
    return [slice(t, min(t + 64, R)) for t in range(0, R, 64)]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_named_edges_are_present_and_decidable(case):
    a = mc.analysis(case)
    r, R, S, v = a.r64, case.R, case.S, case.variant
    n_surv = r.surv.sum(1)
    if case.kind == "empty":
        assert int(n_surv.sum()) == 0 and bool((r.last == 1).all()) and bool((r.depth == 0).all()) and bool(a.decidable.all())
    elif case.kind == "opaque":
        assert bool((n_surv == 1).all()) and bool(a.decidable.all())
        first = r.surv.int().argmax(1)
        assert bool((first == r.evald.int().argmax(1)).all()) and int(first.max()) <= 1      # the first evaluated sample, step 0 or 1
        assert bool((r.last < 1e-3).all())
    elif case.kind == "capacity":
        assert bool((r.last > 1e-3).all())
        assert bool((r.surv == r.evald).all())                        # every evaluated sample survives both thresholds
        if v in ("fourier", "mpi"):                                   # ... and every sample is evaluated: a full tile holds 64 S entries
            assert bool(r.surv.all()) and bool(a.decidable.all())     # (dcvgo, dvgo: the cumdist rule / the step count may sit on its threshold)
    elif case.kind == "faint":      # every sample survives until the ray ends near the last step; its last entries weigh about 2e-4
        assert bool((r.surv == r.evald).all()) and bool(a.decidable.all()) and bool((r.last < 1e-3).all())
        last_w = r.w.gather(1, (n_surv - 1)[:, None])[:, 0]
        assert int(n_surv.min()) >= 38 and float(last_w.max()) < 2.5e-4
    elif case.kind == "one_lane":
        lone = mc.lone_lanes(R)
        for sl, i in zip(_tiles(R), lone):
            alive = r.ran[sl, 2].nonzero().flatten() + sl.start      # rays that take a step after step 1
            assert alive.tolist() == [i], (alive.tolist(), i)
            assert int(r.ran[i].sum()) == (int(r.n[i]) if v == "dvgo" else S) >= 20 and bool(a.decidable[i])
        assert bool(a.decidable.all())
    elif case.kind in ("surfaces", "shell", "geometry") and R >= 64:
        mixed = []                          # lanes go `done` in the middle of a (full) tile
        for sl in _tiles(R)[:R // 64]:
            done = r.last[sl] < 1e-3
            mixed.append(bool(done.any()) and not bool(done.all()))
        # (every tile of the 200- and 323-ray cases; the 37-tile case is there for the launch geometry: most of its tiles)
        assert all(mixed) if R <= 323 else sum(mixed) >= 0.75 * len(mixed), mixed
    if case.kind == "shell":
        for sl in _tiles(R):                # at the same step some rays of the tile are in the shell and others inside
            mixed = r.inner[sl].any(0) & ~r.inner[sl].all(0)
            assert int(mixed.sum()) >= 4, (sl, int(mixed.sum()))
        o_n = (case.rays_o - case.state["scene_center"]) / case.state["scene_radius"]
        assert bool((o_n.abs().amax(1) > 1).all())                   # origins outside the unit cube
        assert bool(((case.rays_d != 0).sum(1) == 1).any())          # axis-parallel, un-normalised directions
    if v == "dcvgo" and case.kind == "shell":
        over, took = r.raw["over"], r.ran & ~r.inner
        took[:, 0] = False
        assert bool((over & took).any()) and bool((~over & took).any())       # the cumdist rule both keeps and skips shell samples
        geom = r.ran & (r.inner | over)
        assert bool((geom & ~r.evald).any())                         # the mask cache's free-space blocks are hit
    if v == "dvgo" and case.kind == "geometry":
        assert bool((case.rays_d[3:6] == 0).any(1).all())            # zero direction components
        miss = slice(8, 16)
        assert bool((r.n[miss] == 1).all()) and int(r.evald[miss].sum()) == 0 and int(n_surv[miss].sum()) == 0
        assert bool(a.decidable[miss].all())
        late = slice(20, 26)                 # origin outside the box, `near` beyond the entry: the first sample lies inside
        lo, hi = mc._box(case.state)
        assert bool((case.rays_o[late, 2] < lo[2]).all()) and bool(r.ran[late, 0].all())
        assert not bool(((r.pos[late, 0] < lo) | (r.pos[late, 0] > hi)).any())
        inside = ((case.rays_o > lo) & (case.rays_o < hi)).all(1)
        assert int(inside.sum()) > R // 2                            # origins inside the box
    if v == "mpi":
        lo, hi = mc._box(case.state)
        on_last = r.evald[:, S - 1] & (r.pos[:, S - 1, 2] == float(hi[2]))
        if case.kind != "opaque":
            assert int(on_last.sum()) > 0                            # the last step lies exactly on the last plane, and is evaluated
        assert bool(a.decided[:, S - 1][on_last].all()) and bool(a.decided[:, 0].all())
        if case.kind == "geometry":
            assert bool((r.ran & ~r.evald).any())                    # rays that leave the box / free-space blocks


def test_mpi_stepsizes_and_fourier_coverage():
    names = set(IDS)
    assert {"mpi-geometry-R200", "mpi-geometry-R200-s1", "mpi-geometry-R200-s0.7"} <= names
    assert sorted({c.S for c in mc.cases("mpi") if c.kind == "geometry"}) == [11, 15, 21]
    for norm in ("inf", "l2"):
        assert {c.kind for c in mc.cases("fourier", 3, norm)} == set(mc.SCENES) | {"shell", "faint"}
        for F in (1, 2, 4, 5):
            assert {c.kind for c in mc.cases("fourier", F, norm)} == {"surfaces", "capacity"}
