"""ugrid_rgbnet_train_forward / _backward (csrc/ugrid_train_mlp.hip) on every kernel shape of their dispatch against a float64
evaluation of the same formula (tests/rgbnet_cases.py), called through _lib as ops.FusedRgbnet calls them, on buffers with guards.

Every cell of rgbnet_cases.SHAPES in both arithmetics (ugrid_tune 'train_mlp' 0 = fp32 MFMA, 1 = bf16x3), at trained-like scales and
at features x 1e4 / g_logits x 1e-6; the default shape at every row count around the 32-row tile and the 128-row weight-gradient
chunk, and at the three row counts where persistent waves take a second tile.  For each: the bound K * max(e32, 2^-23 max |ref64|)
on EVERY element of logits, h1, h2, g_feat and the six weight / bias gradients (K = 8, no ReLU allowance: the builder keeps every
pre-activation 64 bounds away from zero), plus what must hold exactly: zero and dead units give zeros, outputs are written over a NaN
prefill, nothing beyond M rows is read or written, two runs agree, a sample's results depend on nothing but the sample (the same row
in four places; all rows reversed), the first k columns of g_feat do not depend on n_feat_grad, the weight gradients not at all.
Each test prints its ratios err / max(e32, 2^-23 max |ref64|) (`rgbnet-ratio` lines, pytest -s); DESIGN.md section 2b holds the table."""
import pytest
import torch

import rgbnet_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
W_NAMES = ("g_w0", "g_b0", "g_w1", "g_b1", "g_w2", "g_b2")
ROW_NAMES = ("logits", "h1", "h2", "g_feat")
E_NOT_SUPPORTED = 801                                 # hipErrorNotSupported


def _L():
    from unboundednerfpytorch_amd import _lib
    return _lib, _lib.load()


def rows_buf(rows, cols, live, guard, offset=0):
    """[rows + GUARD_ROWS, cols] on the device: `live` in the first rows, `guard` behind them; offset: floats off the allocation's start
    (1 = not 16-byte aligned)"""
    flat = torch.full(((rows + rc.GUARD_ROWS) * cols + offset,), guard, dtype=torch.float32, device=DEV)
    t = flat[offset:].view(rows + rc.GUARD_ROWS, cols)
    t[:rows] = live
    assert t.data_ptr() % 16 == (4 * offset) % 16
    return t


def param_buf(t, offset=0):
    flat = torch.full((t.numel() + offset + 256,), NAN, dtype=torch.float32, device=DEV)
    v = flat[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * offset) % 16
    return v


def flat_buf(n, live, guard, tail=64):
    t = torch.full((n + tail,), guard, dtype=torch.float32, device=DEV)
    t[:n] = live
    return t


class Buffers:
    """everything one forward + backward touches, prefilled: outputs and scratch NaN, rows beyond M of the inputs NaN, rows beyond M of
    the outputs and the tails behind the gradients and the scratch SENTINEL"""

    def __init__(self, mlp_in, width, n_fg, M, feat=None, par=None, g_logits=None, misaligned=None, live=NAN):
        _, L = _L()
        self.mlp_in, self.W, self.n_fg, self.M = mlp_in, width, n_fg, M
        W = width
        self.feat = rows_buf(M, mlp_in, NAN if feat is None else feat.to(DEV), NAN)
        self.g_logits = rows_buf(M, 3, NAN if g_logits is None else g_logits.to(DEV), NAN)
        shapes = [(W, mlp_in), (W,), (W, W), (W,), (3, W), (3,)]
        # the parameters sit in front of 256 NaN floats each: a read beyond a weight array shows in the results
        self.par = [param_buf(torch.zeros(s) if par is None else p, offset=1 if (misaligned == "w2" and i == 4) else 0)
                    for i, (s, p) in enumerate(zip(shapes, par or shapes))]
        self.h1 = rows_buf(M, W, live, rc.SENTINEL)
        self.h2 = rows_buf(M, W, live, rc.SENTINEL, offset=1 if misaligned == "h2" else 0)
        self.logits = rows_buf(M, 3, live, rc.SENTINEL)
        self.g_feat = rows_buf(M, n_fg, live, rc.SENTINEL) if n_fg > 0 else None
        self.grads = [flat_buf(int(torch.Size(s).numel()), live, rc.SENTINEL) for s in shapes]
        self.grad_shapes = shapes
        self.n_scratch = int(L.ugrid_rgbnet_train_scratch_floats(M))
        self.scratch = flat_buf(self.n_scratch, live, rc.SENTINEL, tail=64 * 128)

    def forward(self, mlp_in=None, width=None):
        lib, L = _L()
        p = lib.ptr
        rc_ = L.ugrid_rgbnet_train_forward(p(self.feat), self.M, self.mlp_in if mlp_in is None else mlp_in, *[p(t) for t in self.par],
                                           self.W if width is None else width, p(self.h1), p(self.h2), p(self.logits), lib.stream_of(self.feat))
        torch.cuda.synchronize()
        return int(rc_)

    def backward(self, mlp_in=None, width=None, n_fg=None):
        lib, L = _L()
        p = lib.ptr
        rc_ = L.ugrid_rgbnet_train_backward(p(self.g_logits), p(self.feat), p(self.h1), p(self.h2), self.M, self.mlp_in if mlp_in is None else mlp_in,
                                            self.n_fg if n_fg is None else n_fg, p(self.par[0]), p(self.par[2]), p(self.par[4]),
                                            self.W if width is None else width, p(self.g_feat), *[p(t) for t in self.grads], p(self.scratch),
                                            lib.stream_of(self.feat))
        torch.cuda.synchronize()
        return int(rc_)

    def guards_intact(self):
        M = self.M
        for t in (self.h1, self.h2, self.logits) + ((self.g_feat,) if self.g_feat is not None else ()):
            assert bool((t[M:] == rc.SENTINEL).all())
        for t, s in zip(self.grads, self.grad_shapes):
            assert bool((t[int(torch.Size(s).numel()):] == rc.SENTINEL).all())
        assert bool((self.scratch[self.n_scratch:] == rc.SENTINEL).all())

    def results(self):
        M = self.M
        out = {"logits": self.logits[:M], "h1": self.h1[:M], "h2": self.h2[:M],
               "g_feat": self.g_feat[:M] if self.g_feat is not None else torch.zeros(M, 0)}
        for n, t, s in zip(W_NAMES, self.grads, self.grad_shapes):
            out[n] = t[:int(torch.Size(s).numel())].view(s)
        return {n: t.cpu().clone() for n, t in out.items()}


def run(k, mode, n_fg=None, reverse=False, misaligned=None):
    """one forward + backward of a Case in a tune mode on fresh guarded buffers -> the ten tensors on the host"""
    from unboundednerfpytorch_amd import fourier_render as fr
    n_fg = k.n_fg if n_fg is None else n_fg
    feat, g = (k.feat.flip(0), k.g_logits.flip(0)) if reverse else (k.feat, k.g_logits)
    b = Buffers(k.mlp_in, k.width, n_fg, k.M, feat, k.par, g, misaligned=misaligned)
    try:
        fr.tune("train_mlp", mode)
        assert b.forward() == 0
        b.guards_intact()
        b.h1[k.M:], b.h2[k.M:] = NAN, NAN              # as inputs of the backward: rows beyond M must not be read
        assert b.backward() == 0
    finally:
        fr.tune("train_mlp", 1)
    b.h1[k.M:], b.h2[k.M:] = rc.SENTINEL, rc.SENTINEL
    b.guards_intact()
    return b.results()


def check(k, out, mode, tag="", g_feat_ref=None):
    """finite everywhere, zeros where the zero / dead units put them, the bound on every element of every tensor (every ratio is
    printed before the first assertion)"""
    over = []
    for n in rc.TENSORS:
        ref, e32 = (k.ref64[n], k.e32[n]) if (n != "g_feat" or g_feat_ref is None) else g_feat_ref
        got = out[n]
        assert got.shape == ref.shape and got.dtype == torch.float32, (n, got.shape, ref.shape)
        if ref.numel() == 0:
            continue
        assert bool(torch.isfinite(got).all()), (k.name, n)
        err = float((got.double() - ref).abs().max())
        denom = max(e32, rc.FLOOR * float(ref.abs().max()))
        print("rgbnet-ratio %-28s %-6s %-6s err=%.3g e32=%.3g ratio=%.2f" % (k.name + tag, rc.MODE_NAME[mode], n, err, e32, err / denom))
        if not err <= rc.K_BOUND * denom:
            over.append((n, err, e32, err / denom))
    for t in rc.exact_zero_parts(out, k.width):
        assert not bool(t.any()), k.name
    assert not over, (k.name + tag, rc.MODE_NAME[mode], over)


def same_bits(a, b, names=rc.TENSORS):
    for n in names:
        assert torch.equal(a[n], b[n]), n


def check_cell(k, mode, full=True):
    a = run(k, mode)
    check(k, a, mode)
    same_bits(a, run(k, mode))                                                   # two runs
    for r in k.same_rows[1:]:                                                    # the same sample in other rows: the same bits
        for n in ROW_NAMES:
            assert torch.equal(a[n][r], a[n][0]), (n, r)
    if not full:
        return a
    rev = run(k, mode, reverse=True)                                             # all samples in reverse order
    for n in ROW_NAMES:
        rev[n] = rev[n].flip(0)
        assert torch.equal(rev[n], a[n]), n
    check(k, rev, mode, tag=" reversed")                                         # (the weight gradients: another order of the sample sum)
    # n_feat_grad = mlp_in: the weight gradients do not notice, the first n_feat_grad columns only where another kernel pairs other k
    wide = run(k, mode, n_fg=k.mlp_in)
    check(k, wide, mode, tag=" n_fg=%d" % k.mlp_in, g_feat_ref=k.feat_grad_ref(k.mlp_in))
    same_bits(a, wide, names=("logits", "h1", "h2") + W_NAMES)
    if k.n_fg > 0:
        ka, kw = rc.feat_grad_kernel(mode, k.mlp_in, k.width, k.n_fg), rc.feat_grad_kernel(mode, k.mlp_in, k.width, k.mlp_in)
        if rc.arithmetic_of(ka) == rc.arithmetic_of(kw):
            assert torch.equal(wide["g_feat"][:, :k.n_fg], a["g_feat"]), (ka, kw)
    return a


CELLS = [(s, m, v) for s in rc.SHAPES for m in (0, 1) for v in ("std", "wide")]


@pytest.mark.parametrize("shape,mode,variant", CELLS, ids=["%d/%d/%d-%s-%s" % (*s, rc.MODE_NAME[m], v) for s, m, v in CELLS])
def test_rgbnet_train_matches_fp64(shape, mode, variant):
    check_cell(rc.get(rc.case_of(shape, variant=variant)), mode)


@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("M", rc.M_EDGES)
def test_rgbnet_train_row_counts_around_tiles_and_chunks(M, mode):
    check_cell(rc.get(rc.case_of(rc.DEFAULT, M=M)), mode)


LARGE = [(M, m) for M, modes in rc.LARGE for m in modes]


@pytest.mark.parametrize("M,mode", LARGE, ids=["M%d-%s" % (M, rc.MODE_NAME[m]) for M, m in LARGE])
def test_rgbnet_train_second_tile_and_slab_wrap(M, mode):
    """32768 + 129 rows: more 128-row chunks than the 256 slabs; 65536 + 33: a k_lin_b3 wave's second tile, k_l3_bwd's row chunks
    beyond 8 iterations; 131072 + 33: a k_lin wave's second tile"""
    case = rc.case_of(rc.DEFAULT, M=M)
    try:
        check_cell(rc.get(case), mode, full=False)
    finally:
        if (M, mode) != (rc.LARGE[0][0], 0):      # (the first large case serves two tests)
            rc.forget(case)


@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("which", ["w2", "h2"])
def test_rgbnet_train_misaligned_last_layer_takes_the_mfma_branch(which, mode):
    """w2 or h2 four bytes off the 16-byte grid at width 128: ug_l3_ok is false, the last layer runs on k_lin (n_out = 3, and K = 3 for
    dH2) and k_wgrad (n_out = 3) with 4-tile operands"""
    k = rc.get(rc.case_of(rc.DEFAULT))
    check(k, run(k, mode, misaligned=which), mode, tag=" " + which + "+4B")


@pytest.mark.parametrize("mode", [0, 1], ids=["fp32", "bf16x3"])
def test_fused_rgbnet_op_returns_the_c_level_bits(mode):
    """ops.FusedRgbnet on the default case: the autograd wrapper adds nothing of its own"""
    from unboundednerfpytorch_amd import ops, fourier_render as fr
    k = rc.get(rc.case_of(rc.DEFAULT))
    a = run(k, mode)
    k0 = k.feat[:, :k.n_fg].to(DEV).requires_grad_(True)
    emb = k.feat[:, k.n_fg:].to(DEV)
    par = [p.to(DEV).requires_grad_(True) for p in k.par]
    try:
        fr.tune("train_mlp", mode)
        out = ops.FusedRgbnet.apply(k0, emb, *par)
        out.backward(k.g_logits.to(DEV))
        torch.cuda.synchronize()
    finally:
        fr.tune("train_mlp", 1)
    got = {"logits": out.detach(), "g_feat": k0.grad}
    got.update({n: p.grad for n, p in zip(W_NAMES, par)})
    for n, t in got.items():
        assert torch.equal(t.cpu(), a[n]), n


@pytest.mark.parametrize("width", [128, 30])
def test_rgbnet_train_without_rows(width):
    """M = 0: both calls return 0, the weight and bias gradients come back exactly 0 from a NaN prefill, nothing else is touched"""
    b = Buffers(39, width, 12, 0, live=rc.SENTINEL)
    for t in b.grads:
        t[:-64] = NAN
    keep = [t.clone() for t in (b.h1, b.h2, b.logits, b.g_feat, b.scratch)]
    assert b.forward() == 0 and b.backward() == 0
    b.guards_intact()
    for t, c in zip((b.h1, b.h2, b.logits, b.g_feat, b.scratch), keep):
        assert torch.equal(t, c)
    for n, t in b.results().items():
        if n in W_NAMES:
            assert t.numel() > 0 and not bool(t.any()) and bool(torch.isfinite(t).all()), n


@pytest.mark.parametrize("bad", [dict(width=0), dict(width=129), dict(mlp_in=0), dict(mlp_in=129), dict(n_fg=-1), dict(n_fg=40)],
                         ids=lambda d: "%s=%d" % next(iter(d.items())))
def test_rgbnet_train_rejects_invalid_arguments(bad):
    """width, mlp_in outside 1..128, n_feat_grad outside 0..mlp_in (here mlp_in = 39): hipErrorNotSupported, no output touched"""
    k = rc.get(rc.case_of(rc.DEFAULT, M=33))
    b = Buffers(k.mlp_in, k.width, k.n_fg, k.M, k.feat, k.par, k.g_logits, live=rc.SENTINEL)
    outs = (b.h1, b.h2, b.logits, b.g_feat, b.scratch) + tuple(b.grads)
    keep = [t.clone() for t in outs]
    if "n_fg" not in bad:
        assert b.forward(**bad) == E_NOT_SUPPORTED
    assert b.backward(**bad) == E_NOT_SUPPORTED
    for t, c in zip(outs, keep):
        assert torch.equal(t, c)
