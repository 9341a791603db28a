"""The four march kernels alone (ugrid_render_march: k_march / k_march_ring, ugrid_render_march_dcvgo, _dvgo, _mpi; no shade launch):
their work lists and per-ray outputs on the hand-built scenes of tests/march_cases.py against the float64 march of the same file.

Per case: the list is pre-filled with a byte pattern and the per-ray outputs carry sentinel rows, so every byte the march must not
write is checked; every entry is traced back to its (ray, step) by its position; for the rays whose every decision is decided
(march_cases.Analysis) the entries are exactly the reference's surviving steps, in step-major / lane-ascending order, and positions,
weights, alphainv_last, depth and wsum_mid lie within K * max(e32, floor) of float64; the other rays are compared up to their first
undecided step and held to sanity from there.  FourierGrid cases run at march_waves 6, 7 and 8 and must agree bit for bit.
One `march-ratio` line per case: the worst error of each output, the reference's own fp32 error, their ratio (bound: K = 8).

Measured on an MI355X: profiles/march_worklist/ratios.json."""
import ctypes

import numpy as np
import pytest
import torch

import march_cases as mc

pytestmark = pytest.mark.gpu
WAVES = (6, 7, 8)
FOURIER = [c for norm in ("inf", "l2") for F in (3, 1, 2, 4, 5) for c in mc.cases("fourier", F, norm)]
BOUNDED = [c for v in mc.VARIANTS[1:] for c in mc.cases(v)]


@pytest.fixture
def march_waves():
    from unboundednerfpytorch_amd.fourier_render import tune
    yield lambda w: tune("march_waves", w)
    tune("march_waves", 0)          # 0 = the library's default


class Run:
    """one march call: the work list's bytes and the guarded per-ray outputs, on the host"""

    def __init__(self, ws, last, depth, wmid):
        self.ws, self.last, self.depth, self.wmid = ws.cpu(), last.cpu(), depth.cpu(), None if wmid is None else wmid.cpu()

    def same_as(self, other):
        return (torch.equal(self.ws, other.ws) and torch.equal(self.last, other.last) and torch.equal(self.depth, other.depth)
                and (self.wmid is None or torch.equal(self.wmid, other.wmid)))


class Marcher:
    """the renderer of a case and the march entry point called on it directly (as tools/smi_phases.py does)"""

    def __init__(self, case):
        from unboundednerfpytorch_amd import _lib
        from unboundednerfpytorch_amd.fourier_render import FourierGridRenderer
        self._lib, self.L, self.case = _lib, _lib.load(), case
        self.rend = rend = FourierGridRenderer(case.state, "cuda:0")
        assert (rend.variant or "fourier") == case.variant
        self.t, self.s, S = rend.tables(case.stepsize)
        h = case.h
        assert S == case.S
        self.prm = rend._params(case.R, S, case.stepsize)
        self.vq = rend._variant_params(case.stepsize, S, {"near": case.near} if case.variant == "dvgo" else {})
        # the host parameters march_cases restates are the renderer's
        assert self.prm.interval == np.float32(h.interval) and self.prm.thres == np.float32(case.state["fast_color_thres"])
        if case.variant in ("fourier", "dcvgo"):
            assert torch.equal(self.t.cpu(), h.t) and torch.equal(self.s.cpu(), h.s)
        if case.variant == "dcvgo":
            assert self.vq.dist_thres == np.float32(h.dist_thres)
        if case.variant == "dvgo":
            assert self.vq.stepdist == np.float32(h.stepdist) and self.vq.near_clip == np.float32(h.near)
        if case.variant == "mpi":
            assert self.vq.n_steps == h.n == S
        self.o, self.d = case.rays_o.cuda().contiguous(), case.rays_d.cuda().contiguous()
        self.ws_bytes = int(self.L.ugrid_render_ws_bytes(case.R, S))
        assert self.ws_bytes == mc.worklist_regions(case.R, S)[-1]

    def fresh_list(self):
        return torch.full((self.ws_bytes,), mc.PATTERN, dtype=torch.uint8, device="cuda")

    def march(self, ws=None):
        c, p, L, rend = self.case, self._lib.ptr, self.L, self.rend
        ws = self.fresh_list() if ws is None else ws
        guard = lambda: torch.full((c.R + mc.GUARD_ROWS,), mc.SENTINEL, dtype=torch.float32, device="cuda")
        last, depth, wmid = guard(), guard(), (guard() if c.variant == "dcvgo" else None)
        st = torch.cuda.current_stream().cuda_stream
        if c.variant == "fourier":
            err = L.ugrid_render_march(self.prm, p(self.o), p(self.d), p(self.t), p(self.s), p(rend.density_bricks), p(last), p(depth), p(ws), st)
        elif c.variant == "dcvgo":
            err = L.ugrid_render_march_dcvgo(self.prm, ctypes.byref(self.vq), p(self.o), p(self.d), p(self.t), p(self.s), p(rend.density_bricks),
                                             p(last), p(depth), p(wmid), p(ws), st)
        elif c.variant == "dvgo":
            err = L.ugrid_render_march_dvgo(self.prm, ctypes.byref(self.vq), p(self.o), p(self.d), p(rend.density_bricks), p(last), p(depth), p(ws), st)
        else:
            err = L.ugrid_render_march_mpi(self.prm, ctypes.byref(self.vq), p(self.o), p(self.d), p(rend.density_bricks), p(rend.vp["act_shift"]),
                                           p(last), p(depth), p(ws), st)
        torch.cuda.synchronize()
        assert err == 0, err
        return Run(ws, last, depth, wmid)


def check_untouched(case, run):
    """guard rows, and every byte of the list that is not a count, an entry below its tile's count or a slot below it"""
    R, S = case.R, case.S
    for name, x in (("alphainv_last", run.last), ("depth", run.depth), ("wsum_mid", run.wmid)):
        if x is not None:
            assert bool((x[R:] == mc.SENTINEL).all()), "%s: a guard row behind n_rays was written" % name
            assert bool(torch.isfinite(x[:R]).all()) and bool((x[:R] != mc.SENTINEL).all()), "%s: a ray's output was not written" % name
    nt, cap, oc, oe, os_, total = mc.worklist_regions(R, S)
    buf = run.ws.numpy()
    count = buf[oc:oc + 4 * nt].view(np.int32)
    assert (count >= 0).all() and (count <= cap).all(), "a tile's count was not written: %s" % count       # (the pattern reads negative)
    written = np.zeros(total, dtype=bool)
    written[oc:oc + 4 * nt] = True
    for t in range(nt):
        written[oe + 16 * cap * t: oe + 16 * (cap * t + int(count[t]))] = True
        written[os_ + cap * t: os_ + cap * t + int(count[t])] = True
    stray = np.nonzero(~written & (buf[:total] != mc.PATTERN))[0]
    assert stray.size == 0, "bytes outside the counted entries were written, first at offset %d (count %d, ent %d, slot %d)" % (stray[0], oc, oe, os_)
    return count


def check_against_float64(case, run):
    """structure (exact) and values (K * max(e32, floor)) of one march; returns the march-ratio record"""
    a = mc.analysis(case)
    r, R, S = a.r64, case.R, case.S
    count = check_untouched(case, run)
    tiles = mc.read_worklist(run.ws, R, S)
    lo, hi = [x.double().numpy() for x in mc._box(case.state)]
    thres = float(case.state["fast_color_thres"])
    pos_ref, w_ref, surv = r.pos.numpy(), r.w.numpy(), r.surv.numpy()
    first_und, decidable = a.first_undecided.numpy(), a.decidable.numpy()
    b_pos, b_w = a.bound("pos"), a.bound("w")
    worst = {"pos": 0.0, "w": 0.0}
    per_ray = [[] for _ in range(R)]                     # (step, weight) of every entry, in list order
    for t, (ent, slot) in enumerate(tiles):
        n = len(slot)
        assert n == int(count[t])
        if n == 0:
            continue
        sl = slot.astype(np.int64)
        assert sl.max() < mc.rays_in_tile(R, t), "tile %d: slot %d names no ray of the tile" % (t, sl.max())
        ray = 64 * t + sl
        assert np.isfinite(ent).all()
        d = np.abs(pos_ref[ray] - ent[:, None, :3].astype(np.float64)).max(-1)           # [n, S]: distance to every step of the entry's ray
        step = d.argmin(1)
        assert (np.diff(step) >= 0).all(), "tile %d: the entries are not in step order" % t
        same = np.diff(step) == 0
        assert (np.diff(sl)[same] > 0).all(), "tile %d: lanes do not ascend within a step" % t
        w = ent[:, 3].astype(np.float64)
        assert ((w > thres) & (w <= 1)).all(), "tile %d: weight outside (thres, 1]" % t
        assert ((ent[:, :3] >= lo - b_pos) & (ent[:, :3] <= hi + b_pos)).all(), "tile %d: a position outside the box" % t
        for k in range(n):
            per_ray[ray[k]].append((int(step[k]), w[k], d[k, step[k]]))
    for i in range(R):
        got = per_ray[i]
        ref_steps = np.nonzero(surv[i])[0]
        assert len(got) <= S
        if decidable[i]:
            assert [g[0] for g in got] == ref_steps.tolist(), "ray %d: entries at steps %s, the reference's survivors are %s" % (
                i, [g[0] for g in got], ref_steps.tolist())
            upto = len(got)
        else:      # compared up to the first undecided step; the entries behind it were held to sanity above
            upto = int((ref_steps < first_und[i]).sum())
            assert [g[0] for g in got[:upto]] == ref_steps[:upto].tolist(), "ray %d (undecidable from step %d)" % (i, first_und[i])
            assert all(g[0] >= first_und[i] for g in got[upto:])
        for (j, w, dpos) in got[:upto]:
            worst["pos"], worst["w"] = max(worst["pos"], dpos), max(worst["w"], abs(w - w_ref[i, j]))
            assert dpos <= b_pos, "ray %d step %d: position off by %.3g (bound %.3g)" % (i, j, dpos, b_pos)
            assert abs(w - w_ref[i, j]) <= b_w, "ray %d step %d: weight %.9g, float64 %.9g (bound %.3g)" % (i, j, w, w_ref[i, j], b_w)
    # per-ray outputs of the decidable rays
    dec = a.decidable
    rec = {"case": case.name, "set_aside": round(a.set_aside, 4)}
    step_scale = float(S) if case.variant == "dvgo" else 1.0            # depth = sum w * step index: the floor scales with it
    outs = [("last", run.last, r.last, mc.FLOOR), ("depth", run.depth, r.depth, mc.FLOOR * step_scale)]
    if run.wmid is not None:
        outs.append(("wsum_mid", run.wmid, r.wsum_mid, mc.FLOOR))
    undec = ~dec
    for name, got, ref, floor in outs:
        assert bool(((got[:R] >= 0) & (got[:R] <= max(1.0, step_scale))).all()), name
        err = float((got[:R].double() - ref).abs()[dec].max()) if bool(dec.any()) else 0.0
        denom = max(a.e32[name], floor)
        rec[name] = (err, a.e32[name], err / denom)
        assert err <= mc.K * denom, "%s: err %.3g, e32 %.3g, ratio %.2f" % (name, err, a.e32[name], err / denom)
    rec["pos"] = (worst["pos"], a.e32["pos"] * a.ext, worst["pos"] / (b_pos / mc.K))
    rec["w"] = (worst["w"], a.e32["w"], worst["w"] / (b_w / mc.K))
    print("march-ratio %s %s: " % (case.variant, case.name) + "  ".join(
        "%s err=%.3g e32=%.3g ratio=%.2f" % ((k,) + tuple(rec[k])) for k in ("pos", "w", "last", "depth", "wsum_mid") if k in rec)
        + "  set aside %d of %d rays" % (int(undec.sum()), R))
    return rec


def check_exact_scenes(case, run):
    R = case.R
    if case.kind == "empty":
        count = check_untouched(case, run)
        assert (count == 0).all()
        assert bool((run.last[:R] == 1).all()) and bool((run.depth[:R] == 0).all())          # bit for bit
        assert run.wmid is None or bool((run.wmid[:R] == 0).all())
    if case.kind == "opaque":
        a = mc.analysis(case)
        tiles = mc.read_worklist(run.ws, R, case.S)
        for t, (ent, slot) in enumerate(tiles):
            n = mc.rays_in_tile(R, t)
            assert slot.tolist() == list(range(n)), "tile %d: one entry per ray, in lane order" % t
            alpha = a.r64.alpha[64 * t: 64 * t + n].gather(1, a.r64.surv[64 * t: 64 * t + n].int().argmax(1, keepdim=True))[:, 0]
            assert float((torch.from_numpy(ent[:, 3]).double() - alpha).abs().max()) <= a.bound("w")
    if case.kind == "capacity" and case.variant in ("fourier", "mpi"):
        count = check_untouched(case, run)
        assert count.tolist() == [case.S * mc.rays_in_tile(R, t) for t in range(len(count))]          # a full tile: 64 S, the list's capacity


@pytest.mark.parametrize("case", FOURIER, ids=[c.name for c in FOURIER])
def test_fourier_march(case, march_waves):
    """k_march (6 waves) and k_march_ring (7, 8): bit-identical lists and outputs; one of them against float64; the same call into the
    un-reset list again leaves identical bytes"""
    m = Marcher(case)
    runs = {}
    for w in WAVES:
        march_waves(w)
        runs[w] = m.march()
    for w in WAVES[1:]:
        assert runs[w].same_as(runs[6]), "march_waves %d differs from the 6-wave kernel" % w
    check_against_float64(case, runs[8])
    check_exact_scenes(case, runs[8])
    again = m.march(ws=runs[8].ws.cuda())
    assert again.same_as(runs[8]), "a second march into the same list changed it"


@pytest.mark.parametrize("case", BOUNDED, ids=[c.name for c in BOUNDED])
def test_bounded_march(case):
    m = Marcher(case)
    run = m.march()
    check_against_float64(case, run)
    check_exact_scenes(case, run)
    again = m.march(ws=run.ws.cuda())
    assert again.same_as(run), "a second march into the same list changed it"


@pytest.mark.parametrize("variant", mc.VARIANTS)
def test_empty_march_into_a_full_list_resets_every_count(variant):
    """a recycled work list: `empty` marched into the list `capacity` just filled leaves all counts 0 (and touches nothing else)"""
    by_kind = {c.kind: c for c in mc.cases(variant) if c.R == 200 and c.norm == "inf"}
    full, empty = by_kind["capacity"], by_kind["empty"]
    assert (full.R, full.S) == (empty.R, empty.S)
    filled = Marcher(full).march()
    nt, cap, oc = mc.worklist_regions(full.R, full.S)[:3]
    before = filled.ws.numpy()[oc:oc + 4 * nt].view(np.int32).copy()
    assert (before > 0).all()
    run = Marcher(empty).march(ws=filled.ws.cuda())
    after = run.ws.numpy()[oc:oc + 4 * nt].view(np.int32)
    assert (after == 0).all(), after
    rest = np.ones(run.ws.numel(), dtype=bool)
    rest[oc:oc + 4 * nt] = False
    assert (run.ws.numpy()[rest] == filled.ws.numpy()[rest]).all()
    assert bool((run.last[:full.R] == 1).all()) and bool((run.depth[:full.R] == 0).all())
