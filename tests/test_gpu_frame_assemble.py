"""ugrid_frame_pack / ugrid_frame_assemble alone (csrc/ugrid_frame.hip): pure word permutations, compared as int32 bit patterns.
Inputs carry NaN payloads, -0.0 and denormals; every buffer has sentinel words past its end, which must survive."""
import pytest
import torch

from test_frame_plan import DEALS, SIZES, WORLDS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x5A5A5A5A
PAD = 64
EINVAL = 1


def _lib():
    from unboundednerfpytorch_amd import _lib
    return _lib, _lib.load()


def _padded(n_words, lead=0):
    """int32 [n_words] view of a sentinel-filled buffer, `lead` words into it (lead = 1: the view is not 16-byte aligned)"""
    buf = torch.full((lead + n_words + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf[lead: lead + n_words]


def _intact(buf, lead, n_words):
    return bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n_words:] == SENTINEL).all())


def _bits(n, seed):
    """n random 32-bit patterns (every class of float among them) with a few chosen ones planted"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([-2 ** 31, 0x7FC00001, -0x3EDCBB, 0x7F800000, 1, -2 ** 31 + 1], dtype=torch.int32)   # -0.0, NaNs with payloads, inf, denormals
    k = min(n, special.numel())
    if k:
        x[torch.randperm(n, generator=g)[:k]] = special[:k]
    return x.to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("per", [64, 192])
def test_pack_equals_the_torch_composition(per, lead):
    L, lib = _lib()
    for n in (0, 1, 63, per):
        src_buf, src = _padded(5 * n)
        src.copy_(_bits(5 * n, 10 + n))
        rgb, depth, last = src[: 3 * n].view(n, 3), src[3 * n: 4 * n], src[4 * n:]
        out_buf, out = _padded(5 * per, lead)
        out.fill_(0x11111111)                                              # rows n..per must be WRITTEN as zero
        err = lib.ugrid_frame_pack(L.ptr(rgb) if n else None, L.ptr(depth) if n else None, L.ptr(last) if n else None, n, per,
                                   out.data_ptr(), _stream())
        assert err == 0
        want = torch.zeros(per, 5, dtype=torch.int32, device=DEV)
        want[:n, 0:3], want[:n, 3], want[:n, 4] = rgb, depth, last
        assert torch.equal(out.view(per, 5), want), (n, per, lead)
        assert _intact(out_buf, lead, 5 * per) and _intact(src_buf, 0, 5 * n)
    # the package's wrapper on float tensors
    from unboundednerfpytorch_amd.dist import frame_pack
    f = _bits(5 * 63, 3).view(torch.float32)
    tile = frame_pack(f[: 189].view(63, 3), f[189: 252], f[252:], per)
    assert tile.shape == (per, 5) and torch.equal(tile.view(torch.int32)[:63, 3], f[189: 252].view(torch.int32))
    assert int(tile.view(torch.int32)[63:].abs().max()) == 0


@pytest.mark.parametrize("H,W", SIZES + [(64, 72)])          # 64 x 72: several workgroups
def test_assemble_from_a_gathered_buffer_equals_index_select(H, W):
    """the float at element e of the gathered buffer is the bit pattern of e: a wrong row or column shows as itself"""
    from unboundednerfpytorch_amd.dist import FramePlan, frame_assemble
    L, lib = _lib()
    R = H * W
    for world in WORLDS:
        for deal, dg in DEALS:
            plan = FramePlan(H, W, world, deal, dg)
            n = world * plan.per * 5
            g_buf, g = _padded(n)
            g.copy_(torch.arange(n, dtype=torch.int32, device=DEV))
            for lead in (0, 1):
                out_buf, out = _padded(5 * R, lead)
                err = lib.ugrid_frame_assemble(g.data_ptr(), None, None, None, H, W, world, plan.per, plan.deal_group, int(plan.tile8),
                                               out.data_ptr(), _stream())
                assert err == 0, (world, deal, dg)
                want = torch.index_select(g.view(world * plan.per, 5), 0, plan.src_index().to(DEV))
                assert torch.equal(out.view(R, 5), want), (world, deal, dg, lead)
                assert _intact(out_buf, lead, 5 * R) and _intact(g_buf, 0, n)
            got = frame_assemble(plan, gathered=g.view(torch.float32).view(world * plan.per, 5))
            assert torch.equal(got.view(torch.int32), want)


@pytest.mark.parametrize("H,W", [(8, 8), (16, 24), (64, 72), (13, 7)])
def test_assemble_from_three_arrays_equals_untile_and_cat(H, W):
    from unboundednerfpytorch_amd.dist import FramePlan, frame_assemble
    from unboundednerfpytorch_amd.fourier_render import untile
    L, lib = _lib()
    R = H * W
    src_buf, src = _padded(5 * R)
    src.copy_(_bits(5 * R, H))
    rgb, depth, last = src[: 3 * R].view(R, 3), src[3 * R: 4 * R], src[4 * R:]
    tile8 = H % 8 == 0 and W % 8 == 0
    if tile8:
        want = torch.cat([untile(rgb, H, W), untile(depth, H, W).view(R, 1), untile(last, H, W).view(R, 1)], dim=1)
    else:
        want = torch.cat([rgb, depth.view(R, 1), last.view(R, 1)], dim=1)
    for lead in (0, 1):
        out_buf, out = _padded(5 * R, lead)
        err = lib.ugrid_frame_assemble(None, rgb.data_ptr(), depth.data_ptr(), last.data_ptr(), H, W, 1, R, 0, int(tile8), out.data_ptr(),
                                       _stream())
        assert err == 0
        assert torch.equal(out.view(R, 5), want), lead
        assert _intact(out_buf, lead, 5 * R) and _intact(src_buf, 0, 5 * R)
    got = frame_assemble(FramePlan(H, W, 1), rgb=rgb.view(torch.float32), depth=depth.view(torch.float32), last=last.view(torch.float32))
    assert torch.equal(got.view(torch.int32), want)


def test_sizes_the_32_bit_arithmetic_cannot_hold_are_refused():
    L, lib = _lib()
    out_buf, out = _padded(64)
    p = out.data_ptr()
    assert lib.ugrid_frame_assemble(None, p, p, p, 20726, 20726, 1, 64, 0, 0, p, _stream()) == EINVAL      # 5 H W > 2^31 - 1
    assert lib.ugrid_frame_assemble(p, None, None, None, 16, 24, 8, 1 << 26, 0, 1, p, _stream()) == EINVAL  # 5 world per > 2^31 - 1
    assert lib.ugrid_frame_assemble(p, None, None, None, 13, 7, 1, 128, 0, 1, p, _stream()) == EINVAL       # tile8 on an odd frame
    assert lib.ugrid_frame_assemble(p, None, None, None, 16, 24, 2, 128, 0, 1, p, _stream()) == EINVAL      # rows beyond the buffer
    assert lib.ugrid_frame_pack(p, p, p, 65, 64, p, _stream()) == EINVAL and lib.ugrid_frame_pack(p, p, p, 0, 1 << 29, p, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert _intact(out_buf, 0, 0)                                          # nothing was launched
