"""Cases and plain references for the training rgbnet (csrc/ugrid_train_mlp.hip: ugrid_rgbnet_train_forward / _backward).
TEST INFRASTRUCTURE: tests/test_rgbnet_cases.py (CPU) checks this file, tests/test_gpu_rgbnet_train.py runs the kernels on what
it builds.

The network is  h1 = relu(feat w0^T + b0),  h2 = relu(h1 w1^T + b1),  logits = h2 w2^T + b2  and its derivative for a given
g_logits; `evaluate` writes both out by hand (no autograd) in the dtype it is given.  float64 is the truth, float32 on the CPU
is the yardstick: e32[t] = max |evaluate(float32)[t] - evaluate(float64)[t]| is the reference's OWN fp32 error on tensor t of a
case, and a kernel must stay within K_BOUND * max(e32[t], 2^-23 max |ref64[t]|) of the float64 result on EVERY element.  K_BOUND = 8
is shade_cases.K_BOUND's value for the same two arithmetics (exact fp32 products on v_mfma_f32_32x32x2_f32; bf16x3 with products
at 2^-24) on the same network: the kernel's summation order is another one than the CPU GEMM's (worth about one e32), the bf16x3
products add about as much again, and a maximum over a few thousand elements fluctuates by about 2 x.

No ReLU allowance.  A pre-activation within rounding of zero may land on either side of the ReLU in another summation order, and
that sample then differs by a whole term.  The builder therefore REDRAWS every sample that has a pre-activation with
|z| < margin, margin = 64 x the bound above applied to that layer's pre-activations, until none is left: eight times the error
a kernel is allowed.  It is a condition on the inputs, not a tolerance: no row of any case is excluded from any check.

Exact zeros.  Hidden units ZERO_UNITS(width) of both layers have a weight row and a bias of exactly 0: pre-activation, activation,
incoming weight / bias gradient and (the mask being h > 0) outgoing weight gradient are exactly 0 in any arithmetic.  Unit
DEAD_UNIT(width) has a bias so negative that it is off on every row: the same zeros, behind products that are not zero.
(width >= 8: two zero units + the dead one; width 3..7: one + one; width 1, 2: none -- a live unit has to remain.)

Row locality.  The sample of row 0 (features and g_logits) is repeated in rows 31, 32 and M - 1 (those that exist)."""
import math

import torch

FLOOR = 2.0 ** -23
K_BOUND = 8.0
MARGIN_K = 64.0
# e32 <= E32_REL * max |ref64| on every tensor of every case (tests/test_rgbnet_cases.py): 32 x the floor, so that no bound exceeds
# 8 * 2^-18 = 3.1e-5 of the tensor's largest magnitude -- the relative bound test_fused_rgbnet_matches_torch_linear_layers holds the same
# kernels to against torch's GEMMs.  A case whose own fp32 evaluation is worse than that says nothing about a kernel.
E32_REL = 2.0 ** -18
SENTINEL, GUARD_ROWS = -7.25, 64
FEAT_LIMIT = 8.0                                     # |feat| <= FEAT_LIMIT * scale (N(0, 1) draws; asserted): what the dead unit's bias relies on
TENSORS = ("logits", "h1", "h2", "g_feat", "g_w0", "g_b0", "g_w1", "g_b1", "g_w2", "g_b2")
MODE_NAME = {0: "fp32", 1: "bf16x3"}


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch of ug_lin_launch / ug_wgrad_launch / ug_l3_* and the two entry points, restated for 16-byte aligned buffers
# (what torch allocates).  TEST INFRASTRUCTURE: it names the kernels a cell is MEANT to reach; it cannot observe what ran.
# ---------------------------------------------------------------------------------------------------------------------
def lin_kernel(mode, K, ldx, n_out, ldw, ldy, w_in_major, bias, relu, ldg, x_al=True, w_al=True, yg_al=True):
    """kernel of one ug_lin_launch; ldg = 0: no mask.  x_al / w_al / yg_al: X / W / both Y and G are 16-byte aligned"""
    nt = 1 if n_out <= 32 else 4
    kh = (K + 1) // 2
    if (K <= 4 and w_in_major and not bias and not relu and ldx == K and ldw == n_out and ldy == n_out and ldg in (0, n_out)
            and n_out % 4 == 0 and w_al and yg_al):
        return "k_lin_smallk"
    if mode == 1 and nt == 4 and n_out % 4 == 0 and ldy % 4 == 0 and ldg % 4 == 0 and yg_al:
        al = ldx % 4 == 0 and x_al
        if al and K in (128, 64, 32):
            return "k_lin_b3<%d>" % (K // 16)
        if ldx == K and K <= 48:
            return "k_lin_b3_dense<%d>" % (2 if K <= 32 else 3)
    vec = K == 128 and ldx % 4 == 0 and x_al
    if nt == 4:
        KH = 12 if kh <= 12 else 20 if kh <= 20 else 24 if kh <= 24 else 32 if kh <= 32 else 64
    else:
        KH = 32 if kh <= 32 else 64
    return "k_lin<%d,%d,%s>" % (KH, nt, "vec" if (KH == 64 and vec) else "scalar")


def wgrad_kernel(mode, K):
    if mode == 1 and K > 32:
        return "k_wgrad_b3<2>"
    return "k_wgrad<%d>" % (1 if K <= 32 else 2 if K <= 64 else 4)


def feat_grad_kernel(mode, mlp_in, width, n_fg):
    return lin_kernel(mode, width, width, n_fg, mlp_in, n_fg, 1, 0, 0, 0) if n_fg > 0 else None


def arithmetic_of(kernel):
    """two k_lin instantiations give the same bits per output when they pair the same k (the same KH): NT and VEC change only which
    columns a wave owns and how a row is loaded"""
    return kernel.split(",")[0] if kernel.startswith("k_lin<") else kernel


def kernels(mlp_in, width, n_fg, mode, misaligned=None):
    """the kernels one forward + backward of a shape launches, in launch order (k_wgrad_reduce after every weight gradient).
    misaligned = 'w2' | 'h2': that buffer is not 16-byte aligned, the last layer takes the MFMA branch."""
    W = width
    w_al, h_al = misaligned != "w2", misaligned != "h2"
    out = [lin_kernel(mode, mlp_in, mlp_in, W, mlp_in, W, 0, 1, 1, 0), lin_kernel(mode, W, W, W, W, W, 0, 1, 1, 0, yg_al=h_al)]
    if W % 4 == 0 and w_al and h_al:
        w4 = W >> 2
        out.append("k_l3_fwd<%d>" % (1 if w4 <= 1 else 2 if w4 <= 2 else 4 if w4 <= 4 else 8 if w4 <= 8 else 16 if w4 <= 16 else 32))
        out += ["k_l3_bwd", "k_wgrad_reduce"]
    else:
        out.append(lin_kernel(mode, W, W, 3, W, 3, 0, 1, 0, 0, x_al=h_al, w_al=w_al))
        out += [wgrad_kernel(mode, W), "k_wgrad_reduce", lin_kernel(mode, 3, 3, W, W, W, 1, 0, 0, W, w_al=w_al, yg_al=h_al)]
    out += [wgrad_kernel(mode, W), "k_wgrad_reduce", lin_kernel(mode, W, W, W, W, W, 1, 0, 0, W),
            wgrad_kernel(mode, mlp_in), "k_wgrad_reduce"]
    if n_fg > 0:
        out.append(feat_grad_kernel(mode, mlp_in, W, n_fg))
    return out


# every instantiation ug_lin_launch, ug_wgrad_launch, ug_l3_forward and ug_l3_backward name
ALL_KERNELS = frozenset(
    ["k_lin<%d,4,scalar>" % kh for kh in (12, 20, 24, 32, 64)] + ["k_lin<64,4,vec>", "k_lin<32,1,scalar>", "k_lin<64,1,scalar>", "k_lin<64,1,vec>"]
    + ["k_lin_b3<%d>" % k for k in (2, 4, 8)] + ["k_lin_b3_dense<2>", "k_lin_b3_dense<3>", "k_lin_smallk"]
    + ["k_wgrad<%d>" % n for n in (1, 2, 4)] + ["k_wgrad_b3<2>", "k_wgrad_reduce", "k_l3_bwd"] + ["k_l3_fwd<%d>" % n for n in (1, 2, 4, 8, 16, 32)])

# (mlp_in, width, n_feat_grad): what the cell is in the table for -- the kernels it reaches beyond the default cell's, fp32 mode | bf16x3 mode
# (tests/test_rgbnet_cases.py compares with kernels(); DESIGN.md section 2b lists every cell's full set)
SHAPES = (
    (39, 128, 12),     # default: k_lin<20,4> k_lin<64,4,vec> k_lin<64,1,vec> k_wgrad<2|4> k_l3_fwd<32> k_l3_bwd | k_lin_b3_dense<3> k_lin_b3<8> k_wgrad_b3<2>
    (18, 128, 3),      # k_lin<12,4> k_wgrad<1> | k_lin_b3_dense<2> k_wgrad<1>
    (32, 128, 32),     # k_lin<20,4> k_wgrad<1> | k_lin_b3<2>; n_feat_grad = 32: the widest single-tile input gradient
    (64, 128, 64),     # k_lin<32,4> | k_lin_b3<4> first layer, k_lin_b3<8> input gradient with ldw = mlp_in (4 tiles)
    (128, 128, 128),   # k_lin<64,4,vec> | k_lin_b3<8> first layer, full-width input gradient
    (63, 128, 39),     # k_lin<32,4> in BOTH modes (unaligned rows longer than 48); input gradient 39 columns: k_lin<64,4,vec> in both (39 % 4 != 0)
    (100, 96, 40),     # k_lin<64,4,scalar> for K = 100 and K = 96 in both modes, k_wgrad<4> | k_wgrad_b3<2> with two k-tiles, the second partial
    (48, 128, 0),      # k_lin<24,4> | k_lin_b3_dense<3> at its limit K = 48; g_feat = NULL
    (49, 128, 12),     # k_lin<32,4> | the same: one past the dense-row limit
    (39, 64, 12),      # k_lin<32,4> k_wgrad<2> k_l3_fwd<16> | k_lin_b3<4>
    (39, 40, 12),      # k_lin<20,4> k_l3_fwd<16> | k_lin_b3_dense<3> for the hidden layers (K = width = 40)
    (39, 32, 12),      # nt = 1: k_lin<32,1> for every product in both modes (no bf16x3 k_lin below 33 outputs), k_wgrad<1>(K = 32), k_l3_fwd<8>; first-layer weight gradient k_wgrad<2> | k_wgrad_b3<2>
    (20, 16, 4),       # k_l3_fwd<4>
    (9, 8, 3),         # k_l3_fwd<2>
    (7, 4, 0),         # k_l3_fwd<1>; dH1 = dH2 . W2 with K = 4 on k_lin_smallk (masked); g_feat = NULL
    (8, 4, 8),         # k_lin_smallk without a mask: the input gradient with K = width = 4, n_feat_grad = mlp_in = 8
    (39, 30, 12),      # width % 4 != 0: last layer k_lin<32,1> with n_out = 3, k_wgrad<1>(n_out = 3), dH2 on k_lin<32,1> with K = 3
    (39, 127, 5),      # the same at 4 tiles: k_lin<64,1,scalar>(n_out = 3), k_wgrad<4>(n_out = 3) | k_wgrad_b3<2>(n_out = 3), dH2 on k_lin<12,4> with K = 3
    (5, 3, 5),         # width 3, every product on k_lin<32,1>
    (1, 1, 1),         # one input, one unit
    (24, 128, 12),     # fp32 KH boundaries: kh = 12 -> k_lin<12,4>
    (40, 128, 12),     # kh = 20 -> k_lin<20,4>
    (41, 128, 12),     # kh = 21 -> k_lin<24,4>
    (65, 128, 12),     # kh = 33 -> k_lin<64,4,scalar> with K = 65
)
DEFAULT = (39, 128, 12)
M_CELL = 613                                         # 19 full 32-row tiles + 5 rows; 4 weight-gradient chunks of 128 + 101 rows
M_EDGES = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 512, 513)
# (M, modes): 256 slabs of 128 rows wrap | second tile of k_lin_b3 (256 workgroups x 8 waves x 32 rows) and k_l3_bwd's row chunks past
# 1024 blocks x 64 rows | second tile of k_lin (256 x 16 x 32 rows)
LARGE = ((32768 + 129, (0, 1)), (65536 + 33, (1,)), (131072 + 33, (0,)))


def zero_units(width):
    return (1, width - 1) if width >= 8 else (width - 1,) if width >= 3 else ()


def dead_unit(width):
    return width // 2 if width >= 3 else None


def off_units(width):
    return zero_units(width) + (() if dead_unit(width) is None else (dead_unit(width),))


def exact_zero_parts(out, W):
    """the slices of a result (dict of the ten tensors) that the zero and dead units make exactly 0"""
    off = list(off_units(W))
    return [out["h1"][:, off], out["h2"][:, off], out["g_w0"][off], out["g_b0"][off], out["g_w1"][off], out["g_b1"][off],
            out["g_w1"][:, off], out["g_w2"][:, off]]


# the one or two live units of the narrowest nets are off on every row for most draws of the weights: these shifts of the seed give
# nets whose every tensor has non-zero entries (asserted by tests/test_rgbnet_cases.py for every case)
SEED_SHIFT = {((5, 3, 5), "std"): 1, ((1, 1, 1), "std"): 1}


def case_of(shape, M=M_CELL, variant="std"):
    """(mlp_in, width, n_feat_grad, M, seed, variant); variant 'wide': features x 1e4, g_logits x 1e-6"""
    mlp_in, width, n_fg = shape
    seed = 1000 * mlp_in + 7 * width + n_fg + M + (500000 if variant == "wide" else 0) + SEED_SHIFT.get((shape, variant), 0)
    return (mlp_in, width, n_fg, M, seed, variant)


def case_name(case):
    return "%d/%d/%d M=%d%s" % (case[0], case[1], case[2], case[3], "" if case[5] == "std" else " " + case[5])


def all_cases():
    out = [case_of(s, variant=v) for s in SHAPES for v in ("std", "wide")]
    out += [case_of(DEFAULT, M=m) for m in M_EDGES]
    return out + [case_of(DEFAULT, M=m) for m, _ in LARGE]


# ---------------------------------------------------------------------------------------------------------------------
# the formula
# ---------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def forward(feat, par):
    """pre-activations and activations in the dtype of the arguments"""
    w0, b0, w1, b1, w2, b2 = par
    z1 = feat @ w0.t() + b0
    h1 = torch.relu(z1)
    z2 = h1 @ w1.t() + b1
    h2 = torch.relu(z2)
    return z1, h1, z2, h2, h2 @ w2.t() + b2


@torch.no_grad()
def evaluate(feat, par, g_logits, n_fg, dtype):
    """the ten tensors of TENSORS (+ the pre-activations z1, z2) in `dtype`, the chain rule written out"""
    feat, g_logits, par = feat.to(dtype), g_logits.to(dtype), [p.to(dtype) for p in par]
    w0, b0, w1, b1, w2, b2 = par
    z1, h1, z2, h2, logits = forward(feat, par)
    g_h2 = (g_logits @ w2) * (h2 > 0).to(dtype)
    g_h1 = (g_h2 @ w1) * (h1 > 0).to(dtype)
    return {"logits": logits, "h1": h1, "h2": h2, "z1": z1, "z2": z2,
            "g_feat": g_h1 @ w0[:, :n_fg],
            "g_w0": g_h1.t() @ feat, "g_b0": g_h1.sum(0), "g_w1": g_h2.t() @ h1, "g_b1": g_h2.sum(0),
            "g_w2": g_logits.t() @ h2, "g_b2": g_logits.sum(0)}


def bound_of(e32, ref64, K=K_BOUND):
    return K * max(e32, FLOOR * float(ref64.abs().max())) if ref64.numel() else 0.0


class Case:
    """feat [M, mlp_in], par = [w0, b0, w1, b1, w2, b2] (nn.Linear layout), g_logits [M, 3], all float32; ref64 / ref32: evaluate() in
    the two precisions; e32[t]; redrawn: how many samples the margin condition replaced; same_rows: the rows that hold row 0's sample"""

    def __init__(self, case):
        self.case, self.name = case, case_name(case)
        self.mlp_in, self.width, self.n_fg, self.M, self.seed, self.variant = case
        K, W, M = self.mlp_in, self.width, self.M
        gen = torch.Generator().manual_seed(self.seed)
        fs, gs = (1e4, 1e-6) if self.variant == "wide" else (1.0, 1.0)
        self.feat_scale = fs

        def uniform(shape, fan_in):
            return (torch.rand(shape, generator=gen) * 2 - 1) / math.sqrt(fan_in)

        w0, b0, w1, b1, w2, b2 = (uniform((W, K), K), uniform((W,), K), uniform((W, W), W), uniform((W,), W), uniform((3, W), W),
                                  uniform((3,), W))
        for u in zero_units(W):
            w0[u], b0[u], w1[u], b1[u] = 0.0, 0.0, 0.0, 0.0
        d = dead_unit(W)
        if d is not None:      # below -(the largest pre-activation any admissible input can give)
            b0[d] = -FEAT_LIMIT * fs * float(w0[d].abs().sum())
            h1_max = FEAT_LIMIT * fs * w0.abs().sum(1) + b0.abs()
            b1[d] = -float((w1[d].abs() * h1_max).sum())
        self.par = [w0, b0, w1, b1, w2, b2]
        draw = lambda n: (torch.randn(n, K, generator=gen) * fs, torch.randn(n, 3, generator=gen) * gs)
        feat, g_logits = draw(M)
        # the units the condition is about: not the zero units (exactly 0 by construction: not a rounding question) and not the dead one
        # (asserted below to sit far beyond any margin; its size must not widen the margin of the others)
        live = torch.ones(W, dtype=torch.bool)
        live[list(off_units(W))] = False
        par64 = [p.double() for p in self.par]
        self.redrawn = 0
        self.same_rows = sorted({r for r in (0, 31, 32, M - 1) if r < M})
        while True:
            for r in self.same_rows[1:]:
                feat[r], g_logits[r] = feat[0], g_logits[0]
            z64 = forward(feat.double(), par64)
            z32 = forward(feat, self.par)
            bad = torch.zeros(M, dtype=torch.bool)
            self.margin = []
            for i in (0, 2):
                zl = z64[i][:, live]
                e = float((z32[i][:, live].double() - zl).abs().max())
                margin = MARGIN_K * max(e, FLOOR * float(zl.abs().max()))
                bad |= (zl.abs() < margin).any(1)
                assert d is None or float(z64[i][:, d].max()) < -16 * margin
                self.margin.append(margin)
            n_bad = int(bad.sum())
            if n_bad == 0:
                break
            self.redrawn += n_bad
            feat[bad], g_logits[bad] = draw(n_bad)
        assert float(feat.abs().max()) <= FEAT_LIMIT * fs
        self.feat, self.g_logits = feat, g_logits
        self.ref64 = evaluate(feat, self.par, g_logits, self.n_fg, torch.float64)
        self.ref32 = evaluate(feat, self.par, g_logits, self.n_fg, torch.float32)
        self.e32 = {t: (float((self.ref32[t].double() - self.ref64[t]).abs().max()) if self.ref64[t].numel() else 0.0) for t in self.ref64}

    def bound(self, t, K=K_BOUND):
        return bound_of(self.e32[t], self.ref64[t], K)

    def feat_grad_ref(self, n_fg):
        """(ref64, e32) of g_feat for another n_feat_grad"""
        key = ("g_feat", n_fg)
        if key not in self.__dict__.setdefault("_extra", {}):
            r64 = evaluate(self.feat, self.par, self.g_logits, n_fg, torch.float64)["g_feat"]
            r32 = evaluate(self.feat, self.par, self.g_logits, n_fg, torch.float32)["g_feat"]
            self._extra[key] = (r64, float((r32.double() - r64).abs().max()) if r64.numel() else 0.0)
        return self._extra[key]


_CASES = {}


def get(case):
    """the Case of a case tuple, built once per session"""
    if case not in _CASES:
        _CASES[case] = Case(case)
    return _CASES[case]


def forget(case):
    """drop a large case (a few hundred MB of float64 activations) once its tests are through"""
    _CASES.pop(case, None)
