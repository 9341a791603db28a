"""ugrid_render_shade on hand-built work lists against a float64 evaluation of the same formula (tests/shade_cases.py).

Every triple of UG_SHADE_TRIPLES in every rgbnet arithmetic it accepts, the three kernel geometries at every F, residual colour,
the no-rgbnet kernel, a wide-range scene; bound K * max(e32, 2^-23) on EVERY ray (e32 = the reference's own fp32 error on the case,
K = 8 for fp32 / bf16x3, 32 for fp16x2 -- derivation in shade_cases.py), plus what must hold bit for bit: the geometries agree, a
ray's colour depends on nothing but its own entries in list order, entries beyond a tile's count are never read, rays without
entries are exactly 0, rows beyond n_rays are not written, two runs agree.  Each test prints its measured ratios
err / max(e32, 2^-23) (`shade-ratio` lines, pytest -s); DESIGN.md section 2 holds the table."""

import numpy as np
import pytest
import torch

import shade_cases as sc
import synth
from test_oracle_golden import make_state

pytestmark = pytest.mark.gpu

_PACKED, _DEV_LISTS = {}, {}


def packed(scene):
    if id(scene) not in _PACKED:
        _PACKED[id(scene)] = (scene, sc.Packed(scene))
    return _PACKED[id(scene)][1]


def dev_list(wl, poison=True):
    key = (wl.name, poison)
    if key not in _DEV_LISTS:
        from unboundednerfpytorch_amd import _lib
        ws = wl.bytes(poison=poison)
        assert ws.numel() == _lib.load().ugrid_render_ws_bytes(wl.n_rays, wl.S)
        _DEV_LISTS[key] = (ws.cuda(), wl.viewdirs.cuda().contiguous())
    return _DEV_LISTS[key]


def run(pk, wl, mode, poison=True):
    ws, vd = dev_list(wl, poison)
    err, rgb = pk.shade(ws, vd, wl.n_rays, wl.S, mode)
    assert err == 0, err
    return rgb


def check(tag, pk, wl, mode, K, exact=True):
    """one (scene, list, mode): the bound on every ray + the exact properties; returns the kernel's bits"""
    ref64, e32 = sc.references(pk.sc, wl)
    rgb = run(pk, wl, mode)
    out, guard = rgb[:wl.n_rays], rgb[wl.n_rays:]
    assert torch.isfinite(out).all(), tag
    assert torch.all(guard == sc.SENTINEL), tag                                  # rows >= n_rays are not written
    assert torch.all(out[wl.empty_rays] == 0) and wl.empty_rays.any(), tag       # rays without entries: exactly 0
    for group in wl.same:                                                         # the same entries in other places: the same bits
        for r in group[1:]:
            assert torch.equal(out[group[0]], out[r]), (tag, group, out[group[0]], out[r])
        assert float(out[group[0]].max()) > 0.01
    if exact:
        assert torch.equal(rgb, run(pk, wl, mode)), tag                          # two runs
        assert torch.equal(rgb, run(pk, wl, mode, poison=False)), tag            # nothing beyond the counts is read
    err = float((out.double() - ref64).abs().max())
    denom = max(e32, sc.FLOOR)
    print("shade-ratio %-44s err=%.3g e32=%.3g ratio=%.2f (K=%g)" % (tag + " list " + wl.name, err, e32, err / denom, K))
    assert err <= K * denom, (tag, wl.name, err, e32, err / denom)
    return out


CELLS = [(t, m) for t in sc.TRIPLES for m in sc.modes_of(*t)]


@pytest.mark.parametrize("triple,mode", CELLS, ids=["F%d-C%d-pe%d-%s" % (*t, sc.MODE_NAME[m]) for t, m in CELLS])
def test_shade_matches_fp64(triple, mode):
    pk = packed(sc.scene(*triple))
    assert pk.best_mode == (2 if triple[2] <= 4 else 1)       # the synthetic operands fit fp16x2's range
    for name in sc.MAIN_LISTS:
        check("F%d-C%d-pe%d %s" % (*triple, sc.MODE_NAME[mode]), pk, sc.lists()[name], mode, sc.K_BOUND[mode])


RES_CELLS = [(t, m) for t in sc.RESIDUAL_TRIPLES for m in sc.modes_of(*t)]


@pytest.mark.parametrize("triple,mode", RES_CELLS, ids=["F%d-C%d-pe%d-%s" % (*t, sc.MODE_NAME[m]) for t, m in RES_CELLS])
def test_shade_residual_colour_matches_fp64(triple, mode):
    """rgb = sigmoid(rgbnet([k0[3:], embedding]) + k0[:3]): the epilogue's diffuse term, seen so far only through the DVGO frames"""
    pk = packed(sc.scene(*triple, residual=True))
    for name in sc.MAIN_LISTS:
        check("F%d-C%d-pe%d residual %s" % (*triple, sc.MODE_NAME[mode]), pk, sc.lists()[name], mode, sc.K_BOUND[mode])


def test_shade_without_rgbnet_matches_fp64():
    """k_shade_direct: F = 0, C = 3, mlp_in = 0, rgb = sum w * sigmoid(k0)"""
    pk = packed(sc.scene(0, 3, 0, rgbnet=False))
    for name in sc.MAIN_LISTS + ("five", "many"):
        check("no-rgbnet", pk, sc.lists()[name], 0, sc.K_DIRECT)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp32", "bf16x3", "fp16x2"])
def test_shade_wide_operand_range_matches_fp64(mode):
    """k0 x 10^k with the first layer x 10^-k (as test_rgbnet_fp16x2_range_guard, k = the largest <= 3 at which the reference's own
    fp32 error still meets the CPU condition): fp16x2's power-of-two scales must carry operands far from 1"""
    k = sc.wide_range_k()
    pk = packed(sc.scene(3, 12, 4, wide_k=k))
    assert pk.best_mode == 2
    for name in sc.MAIN_LISTS:
        check("wide-k%d %s" % (k, sc.MODE_NAME[mode]), pk, sc.lists()[name], mode, sc.K_BOUND[mode])


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp32", "bf16x3", "fp16x2"])
def test_shade_one_tile_and_more_tiles_than_waves(mode):
    """n_rays = 5 (one tile) and S = 1 with 256 * 8 + 11 tiles: persistent waves take a second tile and rebuild their embedding table"""
    pk = packed(sc.scene(3, 12, 4))
    for name in ("five", "many"):
        check("F3-C12-pe4 %s" % sc.MODE_NAME[mode], pk, sc.lists()[name], mode, sc.K_BOUND[mode])


@pytest.mark.parametrize("F", [0, 1, 2, 3, 4, 5])
def test_shade_geometries_bit_identical_and_bounded(F):
    """classic (0), 8-wave producer / consumer (1), 12-wave with the lean pass (2; rolling gather set-up at F >= 4): the same bits on
    every list, each within the fp16x2 bound"""
    from unboundednerfpytorch_amd import fourier_render as fr
    pk = packed(sc.scene(F, 12, 4))
    names = sc.MAIN_LISTS + (("five", "many") if F == 3 else ())
    outs = {}
    try:
        for pc in (0, 1, 2):
            fr.tune("shade_pc", pc)
            for name in names:
                outs[pc, name] = check("F%d-C12-pe4 fp16x2 shade_pc=%d" % (F, pc), pk, sc.lists()[name], 2, sc.K_BOUND[2])
    finally:
        fr.tune("shade_pc", 2)
    for name in names:
        assert float(outs[0, name].max()) > 0.05
        for pc in (1, 2):
            assert torch.equal(outs[0, name], outs[pc, name]), (F, pc, name, float((outs[0, name] - outs[pc, name]).abs().max()))


@pytest.mark.parametrize("triple", sc.PROBE_TRIPLES, ids=["F%d-C%d-pe%d" % t for t in sc.PROBE_TRIPLES])
def test_column_probe_isolates_gather_and_embedding(triple):
    """A net that routes three input columns unchanged to the logits (products by 0 and 1 only: exact in fp32 and bf16x3), swept over
    all C + 3 + 6 pe columns: rgb = w * sigmoid(column).  Bound: a quarter (the sigmoid's slope) of 4 x the reference's own fp32 error
    on those columns against float64, floored at 2^-24, plus 2^-23 for the sigmoid and the product.
    The list is 'many', whose rays own at most one entry (4 139 entries in 2 059 tiles, every kind of position, the axis directions):
    the bound has no term for a per-ray sum.  Measured on list 'a' the sweep exceeds it at exactly one place in all five triples --
    the sin(v_z) column, ray 453, which owns 64 entries (the tile whose passes each belong to one ray): 2.234e-7 against 1.788e-7.
    That figure is the fp32 running sum itself: the same 64 products w * sigmoid(column) formed from the float64 column and added in
    list order in fp32 on the CPU differ from the float64 sum by the same 2.23e-7 (the rgbnet, gather and embedding contribute nothing
    visible), so the probe isolates what it is for only where no sum follows it.  The ordered sum is held to the fp64 result by every
    other test of this file."""
    scene, wl = sc.scene(*triple), sc.lists()["many"]
    k32, e32_ = sc.shade_inputs(scene, wl, torch.float32)
    k64, e64_ = sc.shade_inputs(scene, wl, torch.float64)
    x64 = torch.cat([k64, e64_], 1)
    col_err = (torch.cat([k32, e32_], 1).double() - x64).abs().amax(dim=0)      # the reference's own fp32 error per input column
    worst, over = {}, []
    for cols in sc.probe_column_sets(scene.mlp_in):
        pk = sc.Packed(scene, nets=sc.probe_nets(scene.mlp_in, cols))
        # (= shade_reference(float64) with the probe's net, to 1e-15: tests/test_shade_cases.py)
        ref64 = torch.zeros(wl.n_rays, 3, dtype=torch.float64).index_add_(0, wl.ray_id, wl.w.double()[:, None] * torch.sigmoid(x64[:, list(cols)]))
        bound = 0.25 * 4 * max(float(col_err[list(cols)].max()), 2.0 ** -24) + 2.0 ** -23
        for mode in (m for m in sc.modes_of(*triple) if m != 2):
            out = run(pk, wl, mode)[:wl.n_rays]
            err = float((out.double() - ref64).abs().max())
            worst[mode] = max(worst.get(mode, 0.0), err / bound)
            if not err <= bound:
                over.append((cols, sc.MODE_NAME[mode], err, bound))
    for mode, r in worst.items():
        print("shade-ratio probe F%d-C%d-pe%d %s: worst err / bound over the columns = %.2f" % (*triple, sc.MODE_NAME[mode], r))
    assert not over, over


def test_shade_refuses_what_it_does_not_build():
    """non-zero return and an untouched rgb buffer for: an untabulated triple, PE = 8 with fp16x2, C = 9 (with an embedding) with
    fp32, residual colour with C = 3, mlp_width != 128, mlp_in != C + 3 + 6 pe"""
    from unboundednerfpytorch_amd import _lib
    L, wl = _lib.load(), sc.lists()["a"]
    ws, vd = dev_list(wl)

    def refused(pk, mode, **override):
        err, rgb = pk.shade(ws, vd, wl.n_rays, wl.S, mode, **override)
        assert err != 0 and torch.all(rgb == sc.SENTINEL), (err, override)

    pk = packed(sc.scene(3, 12, 4))
    assert L.ugrid_shade_supported(4, 12, 8) == 0 and L.ugrid_shade_supported(3, 12, 2) == 0
    refused(pk, 1, freq_num=4, viewbase_pe=8, mlp_in=12 + 3 + 48)      # untabulated: refused before anything is launched
    refused(pk, 1, viewbase_pe=2, mlp_in=12 + 3 + 12)
    refused(pk, 1, mlp_width=64)
    refused(pk, 1, mlp_in=38)
    refused(pk, 3)
    refused(packed(sc.scene(3, 12, 8)), 2)
    refused(packed(sc.scene(3, 9, 4)), 0)
    refused(packed(sc.scene(0, 9, 4)), 0)
    refused(packed(sc.scene(2, 3, 2)), 1 | _lib.MLP_RESIDUAL)
    assert pk.shade(ws, vd, wl.n_rays, wl.S, 1)[0] == 0               # (the same call without an override is accepted)


def test_render_stats_sums_the_counts():
    from unboundednerfpytorch_amd import _lib
    L = _lib.load()
    for name in ("a", "b", "many", "empty"):
        wl = sc.lists()[name]
        ws, _ = dev_list(wl)
        out = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        _lib.check(L.ugrid_render_stats(_lib.ptr(ws), wl.n_rays, wl.S, _lib.ptr(out), torch.cuda.current_stream().cuda_stream), "stats")
        assert int(out[0].item()) == sum(wl.counts), name
    assert sum(sc.lists()["empty"].counts) == 0
    # an all-empty list shades to exact zeros in every kernel
    for scene, mode in ((sc.scene(3, 12, 4), 2), (sc.scene(2, 3, 2), 1), (sc.scene(0, 3, 0, rgbnet=False), 0)):
        rgb = run(packed(scene), sc.lists()["empty"], mode)
        assert torch.all(rgb[:613] == 0) and torch.all(rgb[613:] == sc.SENTINEL)


def test_real_march_writes_the_layout_the_harness_reads():
    """Bridge: the renderer's own march on a FourierGrid scene (G = 16, 600 rays) -> read_worklist -> step-major, lane-ascending
    tiles whose counts add up to the survivor count -> the float64 reference on that very list bounds the renderer's rgb_marched."""
    from unboundednerfpytorch_amd import fourier_render as fr
    G, F, C, pe, R = 16, 3, 12, 4, 600
    state = make_state(31, G, F, C, pe, "inf", 1e-4, 6.0, 12.0)
    o, d, v = [torch.from_numpy(a) for a in synth.rays(32, R)]
    rend = fr.FourierGridRenderer(state, "cuda:0")
    out = rend(o.cuda(), d.cuda(), v.cuda(), stepsize=0.5, render_depth=True, ray_order="coherent")
    torch.cuda.synchronize()
    S = out["n_max"]
    tiles = sc.read_worklist(rend._ws, R, S)
    assert len(tiles) == 10 and sum(len(s) for _, s in tiles) == rend.survivors_of_last_chunk() > R
    for t, (ent, slot) in enumerate(tiles):
        s = slot.astype(int)
        assert len(s) == 0 or s.max() < sc.rays_in_tile(R, t)
        assert int((np.diff(s) <= 0).sum()) + 1 <= S            # runs of ascending lanes, one per step that kept a sample
        assert np.isfinite(ent).all() and (ent[:, 3] > 1e-4).all() and (np.abs(ent[:, :3]) <= 1.2 + 1e-6).all()
    scene = sc.Scene(F, C, pe, state["k0_grid"], (state["rgbnet_weights"], state["rgbnet_biases"]), lo=(-1.2,) * 3, hi=(1.2,) * 3)
    wl = sc.WorkList("march", R, S, tiles, v)
    ref64, e32 = sc.references(scene, wl)
    assert e32 <= sc.E32_LIMIT
    got = out["rgb_marched"].cpu()
    err, denom = float((got.double() - ref64).abs().max()), max(e32, sc.FLOOR)
    print("shade-ratio bridge G=16 F3-C12-pe4 %s: err=%.3g e32=%.3g ratio=%.2f" % (sc.MODE_NAME[rend.mlp_mode], err, e32, err / denom))
    assert rend.mlp_mode == 2 and err <= sc.K_BOUND[2] * denom, (err, e32)
    assert torch.all(got[wl.empty_rays] == 0)
    # and the hand-written bytes of that list reproduce the march's own bits through the harness's one-call path
    pk = sc.Packed(scene)
    ws2 = sc.write_worklist(R, S, tiles)
    assert ws2.numel() <= rend._ws.numel()
    err2, rgb2 = pk.shade(ws2.cuda(), v.cuda().contiguous(), R, S, 2)
    assert err2 == 0 and torch.equal(rgb2[:R], got)
