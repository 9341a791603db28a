"""CPU checks of the shade harness (tests/shade_cases.py): the work-list bytes, the hand-built lists, the reference, and the
condition that makes the GPU file's bound tight -- every case's own fp32 error stays below 3e-7, so no bound exceeds 1e-5."""
import os
import re

import numpy as np
import pytest
import torch

import shade_cases as sc
from oracle import model_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from unboundednerfpytorch_amd import _lib
    return _lib.load()


def test_triples_are_the_kernels_table(lib):
    """TRIPLES = UG_SHADE_TRIPLES of csrc/ugrid_shade.hip, in its order, and every one is reported as supported"""
    text = open(os.path.join(ROOT, "unboundednerfpytorch_amd", "csrc", "ugrid_shade.hip")).read()
    line = re.search(r"#define UG_SHADE_TRIPLES\(X\)(.*)", text).group(1)
    table = tuple(tuple(int(v) for v in m) for m in re.findall(r"X\((\d+),\s*(\d+),\s*(\d+)\)", line))
    assert table == sc.TRIPLES and len(set(table)) == 14
    assert all(lib.ugrid_shade_supported(*t) == 1 for t in sc.TRIPLES)
    assert set(sc.RESIDUAL_TRIPLES) <= set(table) and set(sc.PROBE_TRIPLES) <= set(table)
    assert all(C >= 9 for _, C, _ in sc.RESIDUAL_TRIPLES)
    n_cells = sum(len(sc.modes_of(*t)) for t in sc.TRIPLES)
    assert n_cells == 14 * 3 - 2 - 2              # pe = 8: no fp16x2 (two triples); C = 9 with an embedding: no fp32 (two triples)


def test_worklist_bytes_match_the_library_and_round_trip(lib):
    for wl in sc.lists().values():
        for poison in (False, True):
            ws = wl.bytes(poison=poison)
            assert ws.dtype == torch.uint8 and ws.numel() == lib.ugrid_render_ws_bytes(wl.n_rays, wl.S)
            back = sc.read_worklist(ws, wl.n_rays, wl.S)
            assert len(back) == len(wl.tiles)
            for (e0, s0), (e1, s1) in zip(wl.tiles, back):
                assert np.array_equal(np.asarray(e0, dtype=np.float32).reshape(-1, 4), e1) and np.array_equal(s0, s1)
    # the regions: 256 B of counters, then count, ent, slot, each aligned to 256 B
    nt, cap, oc, oe, os_, total = sc.worklist_regions(613, 4)
    assert (nt, cap, oc) == (10, 256, 256) and oe == 512 and os_ == 512 + 10 * 256 * 16 and total == os_ + 10 * 256
    assert all(x % 256 == 0 for x in (oc, oe, os_, total))


def test_poison_lies_beyond_the_counts_only():
    wl = sc.lists()["a"]
    nt, cap, oc, oe, os_, total = sc.worklist_regions(wl.n_rays, wl.S)
    clean, dirty = wl.bytes().numpy(), wl.bytes(poison=True).numpy()
    ent_c = clean[oe:oe + nt * cap * 16].view(np.float32).reshape(nt, cap, 4)
    ent_d = dirty[oe:oe + nt * cap * 16].view(np.float32).reshape(nt, cap, 4)
    slot_d = dirty[os_:os_ + nt * cap].reshape(nt, cap)
    assert np.array_equal(clean[:oe], dirty[:oe])                      # counters and counts
    for t, n in enumerate(wl.counts):
        assert np.array_equal(ent_c[t, :n], ent_d[t, :n]) and not np.isnan(ent_d[t, :n]).any()
        assert np.isnan(ent_d[t, n:]).all() and (ent_c[t, n:] == 0).all()
        if n < cap:
            ray = 64 * t + int(slot_d[t, n])
            assert (slot_d[t, n:] == slot_d[t, n]).all() and ray < wl.n_rays and bool(wl.empty_rays[ray])


def test_lists_hold_the_shapes_the_kernels_can_get_wrong():
    L = sc.lists()
    a, b = L["a"], L["b"]
    assert a.n_rays == b.n_rays == 613 and len(a.tiles) == 10 and sc.rays_in_tile(613, 9) == 37 and 613 % 8 != 0
    counts = a.counts + b.counts
    assert set((0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 256)) <= set(counts)
    assert a.counts[2] == 1 and int(a.tiles[2][1][0]) == 63                                      # a lone survivor in slot 63
    one_ray = a.tiles[7][1]
    assert len(one_ray) == 137 and all(len(set(one_ray[i:i + 32].tolist())) == 1 for i in range(0, 137, 32))
    assert a.tiles[8][1].tolist() == [10, 11] * 35                                               # two rays alternating
    for wl in (a, b):                                                                            # the partial last tile
        assert 0 < wl.counts[9] and int(wl.tiles[9][1].max()) < 37
    march = b.tiles[0][1].astype(int)                                                            # step-major, lanes ascending
    assert int((np.diff(march) <= 0).sum()) + 1 == sc.S_SMALL and 64 < len(march) < 256
    # the shared sequence: slot 0 of tile 0, slot 63 of the full tile, the partial last tile; same entries, same view direction
    (ra, rb, rc), = a.same
    assert (ra, rb, rc) == (0, 6 * 64 + 63, 9 * 64 + 36) and a.counts[6] == 256
    seqs = [torch.cat([a.pos[a.ray_id == r], a.w[a.ray_id == r, None]], 1) for r in (ra, rb, rc)]
    assert seqs[0].shape == (sc.SEQ_LEN, 4) and torch.equal(seqs[0], seqs[1]) and torch.equal(seqs[0], seqs[2])
    assert torch.equal(a.viewdirs[ra], a.viewdirs[rb]) and torch.equal(a.viewdirs[ra], a.viewdirs[rc])
    where = [np.nonzero(a.tiles[t][1] == s)[0] for t, s in ((0, 0), (6, 63), (9, 36))]
    assert len(set(tuple(w % 32) for w in where)) == 3                                           # in other lanes of other passes
    five, many = L["five"], L["many"]
    assert five.n_rays == 5 and len(five.tiles) == 1 and five.S == 4
    assert many.S == 1 and len(many.tiles) == 256 * 8 + 11 and 1.5 < many.pos.shape[0] / len(many.tiles) < 2.5 and 0 in many.counts
    assert len(set(many.ray_id.tolist())) == many.pos.shape[0]                                   # at most one entry per ray: no sum
    assert L["empty"].pos.shape[0] == 0
    lo, hi = torch.tensor(sc.BOX_LO), torch.tensor(sc.BOX_HI)
    for wl in L.values():
        assert max(wl.counts) <= 64 * wl.S
        assert torch.all(wl.pos >= lo) and torch.all(wl.pos <= hi)
        assert float((wl.viewdirs.double().norm(dim=1) - 1).abs().max()) < 1e-6
        per_ray = torch.zeros(wl.n_rays, dtype=torch.float64).index_add_(0, wl.ray_id, wl.w.double())
        assert float(per_ray.max()) <= 1.0 and not (wl.w < 0).any()
    for wl in (a, b, many):
        is_axis = (wl.viewdirs.abs().amax(dim=1) == 1) & (wl.viewdirs.abs().sum(dim=1) == 1)
        assert int(is_axis.sum()) == 6 and not wl.empty_rays[is_axis].any()                      # the axis directions are used
        assert sorted(wl.viewdirs[is_axis].tolist()) == sorted(sc.AXIS_DIRS.tolist())
    for wl in (a, b):
        assert (wl.w == 0).any() and (wl.w == np.float32(1e-12)).any()
        # corners / edges / faces, exact vertices and cell centres are all present
        g1 = torch.tensor(sc.GRID, dtype=torch.float64) - 1
        ix = (wl.pos.double() - lo.double()) / (hi.double() - lo.double()) * g1
        frac = (ix - ix.round()).abs()
        assert int((frac.amax(dim=1) < 1e-6).sum()) > 50 and int(((frac - 0.5).abs().amax(dim=1) < 1e-6).sum()) > 50
        on_box = ((wl.pos == lo) | (wl.pos == hi)).any(dim=1)
        assert int(on_box.sum()) > 50


def test_reference_is_the_plain_formula():
    """shade_reference against a sample-by-sample evaluation written out here (float64), with and without residual colour, and the
    column probe's net against w * sigmoid(column)"""
    wl = sc.lists()["a"]
    for s in (sc.scene(3, 12, 4), sc.scene(0, 9, 4, residual=True), sc.scene(0, 3, 0, rgbnet=False)):
        ref = sc.shade_reference(s, wl, torch.float64)
        k0, emb = sc.shade_inputs(s, wl, torch.float64)
        want = torch.zeros(wl.n_rays, 3, dtype=torch.float64)
        if s.nets is None:
            logits = k0
        else:
            (w0, w1, w2), (b0, b1, b2) = [[x.double() for x in part] for part in s.nets]
            x = torch.cat([k0[:, 3:] if s.residual else k0, emb], 1)
            h = torch.relu(torch.relu(x @ w0.T + b0) @ w1.T + b1) @ w2.T + b2
            logits = h + (k0[:, :3] if s.residual else 0)
        val = wl.w.double()[:, None] / (1 + torch.exp(-logits))
        for i in range(wl.pos.shape[0]):
            want[wl.ray_id[i]] += val[i]
        assert float((ref - want).abs().max()) < 1e-14
        assert torch.all(ref[wl.empty_rays] == 0) and wl.empty_rays.any()
    s = sc.scene(3, 12, 4)
    k0, emb = sc.shade_inputs(s, wl, torch.float64)
    x = torch.cat([k0, emb], 1)
    sets = sc.probe_column_sets(s.mlp_in)
    assert len(sets) == 13 and sorted(set(c for cs in sets for c in cs)) == list(range(39))
    for cols in (sets[0], sets[5], sets[-1]):
        ref = sc.shade_reference(s, wl, torch.float64, nets=sc.probe_nets(s.mlp_in, cols))
        want = torch.zeros(wl.n_rays, 3, dtype=torch.float64).index_add_(0, wl.ray_id, wl.w.double()[:, None] * torch.sigmoid(x[:, list(cols)]))
        assert float((ref - want).abs().max()) < 1e-15
    # the features are the oracle's: a vertex position returns the grid value of that vertex (F = 0)
    s0 = sc.scene(0, 12, 4)
    X, Y, Z = sc.GRID
    p = torch.tensor([[sc.BOX_LO[0] + 2 * 2.0 / (X - 1), sc.BOX_LO[1] + 3 * 2.0 / (Y - 1), sc.BOX_LO[2] + 5 * 3.0 / (Z - 1)]], dtype=torch.float64)
    got = model_oracle.fourier_grid_query(s0.kg.double(), p, s0.lo.double(), s0.hi.double(), 0)
    assert float((got[0] - s0.kg[0, :, 2, 3, 5].double()).abs().max()) < 1e-12


def test_every_case_meets_the_fp32_condition():
    """the reference's own fp32 error on every (scene, list) the GPU file bounds: <= 3e-7, so K * max(e32, 2^-23) <= 1e-5"""
    torch.set_num_threads(1)
    worst = 0.0
    scenes = sc.all_scenes()
    assert len(scenes) == 14 + 3 + 2
    for tag, s in scenes:
        for name in sc.MAIN_LISTS:
            e32 = sc.references(s, sc.lists()[name])[1]
            print("e32 %-24s list %s: %.3g" % (tag, name, e32))
            assert 0 < e32 <= sc.E32_LIMIT, (tag, name, e32)
            worst = max(worst, e32)
    for name in ("five", "many"):
        e32 = sc.references(sc.scene(3, 12, 4), sc.lists()[name])[1]
        print("e32 F3-C12-pe4 list %s: %.3g" % (name, e32))
        assert 0 < e32 <= sc.E32_LIMIT, (name, e32)
        worst = max(worst, e32)
    assert max(sc.K_BOUND.values()) * max(worst, sc.FLOOR) <= 1e-5
    assert 1 <= sc.wide_range_k() <= 3
