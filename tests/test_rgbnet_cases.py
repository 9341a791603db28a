"""CPU checks of the training rgbnet's test harness (tests/rgbnet_cases.py): the hand-written formula against autograd, the margin
condition that lets the GPU file go without a ReLU allowance, the exact-zero units, and the condition that keeps the bound tight --
every tensor's own fp32 error stays below E32_REL of its largest magnitude."""
import os
import re

import pytest
import torch

import rgbnet_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = rc.all_cases()
W_NAMES = ("g_w0", "g_b0", "g_w1", "g_b1", "g_w2", "g_b2")


def test_shape_table_holds_the_cells_and_reaches_every_kernel():
    need = [(39, 128, 12), (18, 128, 3), (32, 128, 32), (64, 128, 64), (128, 128, 128), (63, 128, 39), (100, 96, 40), (48, 128, 0),
            (49, 128, 12), (39, 64, 12), (39, 40, 12), (39, 32, 12), (20, 16, 4), (9, 8, 3), (7, 4, 0), (39, 30, 12), (39, 127, 5),
            (5, 3, 5), (1, 1, 1), (24, 128, 12), (40, 128, 12), (41, 128, 12), (65, 128, 12)]
    assert set(need) <= set(rc.SHAPES) and len(set(rc.SHAPES)) == len(rc.SHAPES)
    assert rc.M_CELL == 19 * 32 + 5 == 4 * 128 + 101
    reached = {k for s in rc.SHAPES for m in (0, 1) for k in rc.kernels(*s, m)}
    reached |= {k for m in (0, 1) for mis in ("w2", "h2") for k in rc.kernels(*rc.DEFAULT, m, misaligned=mis)}
    assert reached == rc.ALL_KERNELS, (reached ^ rc.ALL_KERNELS)
    # ALL_KERNELS against the source: every template argument list a launch macro or a launch names
    text = open(os.path.join(ROOT, "unboundednerfpytorch_amd", "csrc", "ugrid_train_mlp.hip")).read()
    host = text[text.index("static inline int ug_lin_launch"):]
    src = {"k_lin<%s,%s,%s>" % (a, b, {"true": "vec", "false": "scalar"}[c]) for a, b, c in re.findall(r"UG_LIN_GO\((\d+), (\d), (true|false)\)", host)}
    src |= {"k_lin_b3<%s>" % a for a in re.findall(r"UG_LINB_GO\((\d)\)", host)} | {"k_lin_b3_dense<%s>" % a for a in re.findall(r"UG_LINB_DENSE\((\d)\)", host)}
    src |= {"%s<%s>" % m for m in re.findall(r"HIP_KERNEL_NAME\((k_wgrad(?:_b3)?)<(\d)>\)", host)}
    src |= {"k_l3_fwd<%s>" % a for a in re.findall(r"UG_L3F\((\d+)\);", host)}
    src |= {k for k in ("k_lin_smallk", "k_l3_bwd", "k_wgrad_reduce") if "hipLaunchKernelGGL(%s," % k in host}
    assert src == rc.ALL_KERNELS, (src ^ rc.ALL_KERNELS)


def test_the_cells_reach_what_the_table_says():
    """the kernels named beside the entries of SHAPES, per mode (fp32, bf16x3)"""
    K = lambda s, m: set(rc.kernels(*s, m))
    assert {"k_lin<20,4,scalar>", "k_lin<64,4,vec>", "k_lin<64,1,vec>", "k_wgrad<2>", "k_wgrad<4>", "k_l3_fwd<32>", "k_l3_bwd"} <= K((39, 128, 12), 0)
    assert {"k_lin_b3_dense<3>", "k_lin_b3<8>", "k_wgrad_b3<2>", "k_lin<64,1,vec>"} <= K((39, 128, 12), 1)
    assert {"k_lin_b3_dense<2>", "k_wgrad<1>"} <= K((18, 128, 3), 1) and "k_lin<12,4,scalar>" in K((18, 128, 3), 0)
    assert "k_lin_b3<2>" in K((32, 128, 32), 1) and rc.feat_grad_kernel(1, 32, 128, 32) == "k_lin<64,1,vec>"
    assert "k_lin_b3<4>" in K((64, 128, 64), 1) and rc.feat_grad_kernel(1, 64, 128, 64) == "k_lin_b3<8>"
    assert K((128, 128, 128), 1) == {"k_lin_b3<8>", "k_wgrad_b3<2>", "k_wgrad_reduce", "k_l3_fwd<32>", "k_l3_bwd"}
    assert "k_lin<32,4,scalar>" in K((63, 128, 39), 1) and rc.feat_grad_kernel(1, 63, 128, 39) == "k_lin<64,4,vec>"
    assert not any(k.startswith("k_lin_b3") for k in K((100, 96, 40), 1)) and "k_lin<64,4,scalar>" in K((100, 96, 40), 1)
    assert "k_lin_b3_dense<3>" in K((48, 128, 0), 1) and "k_lin<24,4,scalar>" in K((48, 128, 0), 0)
    assert "k_lin<32,4,scalar>" in K((49, 128, 12), 1)
    assert {"k_lin_b3<4>", "k_l3_fwd<16>"} <= K((39, 64, 12), 1) and rc.kernels(39, 40, 12, 1)[1] == "k_lin_b3_dense<3>"
    for s, l3 in (((39, 32, 12), 8), ((20, 16, 4), 4), ((9, 8, 3), 2), ((7, 4, 0), 1)):
        for m in (0, 1):
            assert "k_l3_fwd<%d>" % l3 in K(s, m) and not any(",4," in k or "b3<" in k and "wgrad" not in k for k in K(s, m))
    assert rc.kernels(7, 4, 0, 1).count("k_lin_smallk") == 1 and rc.kernels(8, 4, 8, 1).count("k_lin_smallk") == 2
    for s in ((39, 30, 12), (39, 127, 5), (5, 3, 5), (1, 1, 1)):
        assert not any(k.startswith("k_l3") for m in (0, 1) for k in K(s, m))
    assert {"k_lin<64,1,scalar>", "k_lin<12,4,scalar>"} <= K((39, 127, 5), 0)
    for s, kh in (((24, 128, 12), 12), ((40, 128, 12), 20), ((41, 128, 12), 24), ((65, 128, 12), 64)):
        assert rc.kernels(*s, 0)[0] == "k_lin<%d,4,scalar>" % kh
    # w2 or h2 off the 16-byte grid at width 128: the MFMA last layer, n_out = 3 weight gradient, K = 3 product
    # (a misaligned w2 leaves the K = 3 product on the bf16x3 dense-row kernel, which reads W with scalar loads)
    mis = rc.kernels(39, 128, 12, 1, misaligned="h2")
    assert mis[1] == "k_lin<64,4,vec>" and mis[2] == "k_lin<64,1,scalar>" and mis[3] == "k_wgrad_b3<2>" and mis[5] == "k_lin<12,4,scalar>"
    mis = rc.kernels(39, 128, 12, 1, misaligned="w2")
    assert mis[1] == "k_lin_b3<8>" and mis[2] == "k_lin<64,1,vec>" and mis[3] == "k_wgrad_b3<2>" and mis[5] == "k_lin_b3_dense<2>"
    assert rc.kernels(39, 128, 12, 0, misaligned="w2")[3:6] == ["k_wgrad<4>", "k_wgrad_reduce", "k_lin<12,4,scalar>"]
    assert rc.arithmetic_of("k_lin<64,1,vec>") == rc.arithmetic_of("k_lin<64,4,scalar>") != rc.arithmetic_of("k_lin<32,1,scalar>")


@pytest.mark.parametrize("case", CASES, ids=[rc.case_name(c).replace(" ", "-") for c in CASES])
def test_case(case):
    k = rc.get(case)
    try:
        _check_case(k)
    finally:
        if k.M > 5000:
            rc.forget(case)


def _check_case(k):
    W, M = k.width, k.M
    assert k.feat.shape == (M, k.mlp_in) and k.g_logits.shape == (M, 3) and k.feat.dtype == k.g_logits.dtype == torch.float32
    assert [tuple(p.shape) for p in k.par] == [(W, k.mlp_in), (W,), (W, W), (W,), (3, W), (3,)]
    for r in k.same_rows:
        assert torch.equal(k.feat[r], k.feat[0]) and torch.equal(k.g_logits[r], k.g_logits[0])
    assert k.same_rows == sorted({r for r in (0, 31, 32, M - 1) if r < M})
    # ---- the hand-written formula is the derivative: autograd in float64 on the same nn.Sequential
    net = torch.nn.Sequential(torch.nn.Linear(k.mlp_in, W), torch.nn.ReLU(), torch.nn.Linear(W, W), torch.nn.ReLU(), torch.nn.Linear(W, 3)).double()
    with torch.no_grad():
        for p, v in zip(net.parameters(), k.par):
            p.copy_(v.double())
    x = k.feat.double().requires_grad_(True)
    out = net(x)
    out.backward(k.g_logits.double())
    auto = {"logits": out.detach(), "g_feat": x.grad[:, :k.n_fg]}
    auto.update({n: p.grad for n, p in zip(W_NAMES, net.parameters())})
    for n, a in auto.items():
        r = k.ref64[n]
        assert r.dtype == torch.float64 and r.shape == a.shape
        assert float((r - a).abs().max()) <= 1e-12 * float(a.abs().max()) if a.numel() else True, n
    # ---- the margin condition: no pre-activation of a live unit within 64 bounds of zero, hence the same ReLU pattern in float32
    live = torch.ones(W, dtype=torch.bool)
    live[list(rc.off_units(W))] = False
    for z, h, margin in (("z1", "h1", k.margin[0]), ("z2", "h2", k.margin[1])):
        zl = k.ref64[z][:, live]
        e = float((k.ref32[z][:, live].double() - zl).abs().max())
        assert margin == rc.MARGIN_K * max(e, rc.FLOOR * float(zl.abs().max())) and margin > 0
        assert float(zl.abs().min()) >= margin
        assert torch.equal(k.ref32[h] > 0, k.ref64[h] > 0)                       # every unit of every row
        assert torch.equal(k.ref32[z] > 0, k.ref64[z] > 0)
    # ---- exact zeros, in float32 as in float64
    off, zero = list(rc.off_units(W)), list(rc.zero_units(W))
    assert len(zero) == (2 if W >= 8 else 1 if W >= 3 else 0) and len(off) == len(zero) + (1 if W >= 3 else 0) and len(off) < W
    for ref in (k.ref32, k.ref64):
        assert not bool(ref["z1"][:, zero].any()) and not bool(ref["z2"][:, zero].any())
        assert not off or float(ref["z1"][:, off].max()) <= 0 and float(ref["z2"][:, off].max()) <= 0
        for t in rc.exact_zero_parts(ref, W):
            assert not bool(t.any())
    # ---- the yardstick means something: every tensor has entries, and its own fp32 error is small beside them
    for n in rc.TENSORS:
        r = k.ref64[n]
        if r.numel() == 0:
            assert n == "g_feat" and k.n_fg == 0
            continue
        top = float(r.abs().max())
        assert top > 0 and torch.isfinite(r).all(), n
        assert k.e32[n] <= rc.E32_REL * top, (n, k.e32[n], top)
        assert k.bound(n) == rc.K_BOUND * max(k.e32[n], rc.FLOOR * top) <= 8 * rc.E32_REL * top


def test_wide_variant_scales_and_case_ids():
    a, b = rc.get(rc.case_of(rc.DEFAULT)), rc.get(rc.case_of(rc.DEFAULT, variant="wide"))
    assert 1e4 < float(b.feat.abs().max()) <= 8e4 and float(a.feat.abs().max()) <= 8
    assert float(b.g_logits.abs().max()) < 1e-5 < 1 < float(a.g_logits.abs().max())
    assert len({c[4] for c in CASES}) == len(CASES)                                # another seed per case
    assert [m for m, _ in rc.LARGE] == [32768 + 129, 65536 + 33, 131072 + 33]
    assert len(CASES) == 2 * len(rc.SHAPES) + len(rc.M_EDGES) + 3
