"""No GPU: what tests/test_gpu_self_attn_bwd.py rests on before the kernel runs -- over the whole case table of
``tests/self_attn_bwd_cases.py`` the fp32 / T emulation of the attention backward core in its masked self-attention form sits inside the
derived bound (worst |d| / bound <= 1: a condition, not a figure), every named mutant leaves it on its named cases, the float64 reference is
torch.autograd's gradient of a float64 masked softmax attention, and ``mra_debug_self_attention_bwd`` refuses bad arguments before any
launch."""
import functools

import pytest
import torch

import qformer_kernel_cases as K
import self_attn_bwd_cases as SB
from mraudio_amd import _lib

DTYPES = (torch.float16, torch.bfloat16)
ITEMS, HEADS = 3, 2
MASKED = ("ragged", "holes", "zero_row")


@functools.lru_cache(maxsize=None)
def case(kind, S, dtype, mask_kind, chained=False):
    return SB.build(kind, ITEMS, HEADS, S, dtype, mask_kind, chained=chained)


def _emulated(c, mutant=None):
    return SB.emulate(c.q, c.k, c.v, c.o, c.d_o, c.lse, c.mask, mutant=mutant)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("S", SB.BWD_S)
def test_the_emulation_sits_inside_the_bound(S, dtype):
    worst = [(0.0, None)] * 3
    for kind in SB.FAMILIES:
        for mk in SB.MASK_KINDS:
            c = case(kind, S, dtype, mk)
            r = SB.ratios(_emulated(c), c.ref, c.bound)
            worst = [max(w, (x, (kind, mk))) for w, x in zip(worst, r)]
    print(f"emulation S={S} {dtype}: |d| / bound dq {worst[0][0]:.3f} at {worst[0][1]}, dk {worst[1][0]:.3f} at {worst[1][1]}, "
          f"dv {worst[2][0]:.3f} at {worst[2][1]}")
    assert all(w[0] <= 1.0 for w in worst), worst


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("S", (33, 160, 257))
def test_the_emulated_forward_and_backward_chain_sits_inside_the_chained_bound(S, dtype):
    """ctx and lse from the emulation of attn_kernel (qformer_kernel_cases.attn_emulate) instead of the rounded float64 values."""
    worst = [(0.0, None)] * 3
    for kind in SB.FAMILIES:
        for mk in SB.MASK_KINDS:
            c = case(kind, S, dtype, mk, True)
            ctx, lse = K.attn_emulate(c.q, c.k, c.v, c.mask)
            r = SB.ratios(SB.emulate(c.q, c.k, c.v, ctx, c.d_o, lse, c.mask), c.ref, c.chained_bound)
            worst = [max(w, (x, (kind, mk))) for w, x in zip(worst, r)]
    print(f"chained emulation S={S} {dtype}: |d| / bound dq {worst[0][0]:.3f}, dk {worst[1][0]:.3f}, dv {worst[2][0]:.3f}")
    assert all(w[0] <= 1.0 for w in worst), worst


# mutant: (S values, mask kinds) on which it must leave the bound, in both families and both dtypes (self_attn_bwd_cases' docstring)
MUTANT_CASES = {
    "mask_ignored": ((33, 65, 160, 257), MASKED),
    "mask_item0": ((33, 65, 160, 257), ("ragged",)),
    "mask_block0": ((33, 65, 160, 257), MASKED),
    "qblock0": ((33, 65, 160, 257), SB.MASK_KINDS),
    "round2_dropped": ((129, 160, 161, 257), SB.MASK_KINDS),
    "qclamp_counted": ((33, 41, 65, 129, 161), SB.MASK_KINDS),
    "masked_q_zero": ((33, 65, 160, 257), MASKED),
}


@pytest.mark.parametrize("mutant", SB.MUTANTS)
def test_mutants_leave_the_bound(mutant):
    sizes, masks = MUTANT_CASES[mutant]
    least = (float("inf"), None)
    for dtype in DTYPES:
        for S in sizes:
            for kind in SB.FAMILIES:
                for mk in masks:
                    c = case(kind, S, dtype, mk)
                    r = max(SB.ratios(_emulated(c, mutant), c.ref, c.bound))
                    least = min(least, (r, (kind, S, mk, dtype)))
                    assert r > 1.0, (mutant, kind, S, mk, dtype, r)
    print(f"mutant {mutant}: least worst |d| / bound over its cases {least[0]:.1f} at {least[1]}")


def test_the_mutant_table_names_every_mutant():
    assert set(MUTANT_CASES) == set(SB.MUTANTS)


@pytest.mark.parametrize("mask_kind", SB.MASK_KINDS)
def test_the_reference_is_autograd_of_a_float64_masked_attention(mask_kind):
    S = 65
    q, k, v = (t.double().requires_grad_(True) for t in K.make_attn("peaked", ITEMS, HEADS, S, torch.float16))
    d_o = SB.make_grad(ITEMS, HEADS, S, torch.float16)
    mask = K.make_mask(mask_kind, ITEMS, S)
    s = q @ k.transpose(-1, -2) / 8
    if mask is not None:
        s = s + ((1 - mask).double() * -10000.0)[:, None, None, :]
    o = torch.softmax(s, -1) @ v
    o.backward(d_o.double())
    r = SB.bwd_ref(q.detach().half(), k.detach().half(), v.detach().half(), d_o, mask)
    assert torch.allclose(r.o, o.detach(), rtol=0, atol=1e-13)
    for name, got, want in (("dq", r.dq, q.grad), ("dk", r.dk, k.grad), ("dv", r.dv, v.grad)):
        assert want.abs().max().item() > 0
        assert ((got - want).norm() / want.norm()).item() <= 1e-10, (name, mask_kind)
    # the lse the kernels exchange: log2 units, mask included
    y = r.s * SB.LOG2E
    ymax = y.amax(-1, keepdim=True)
    assert torch.allclose(r.lse, torch.log2(torch.exp2(y - ymax).sum(-1)) + ymax.squeeze(-1), rtol=0, atol=1e-9)


def test_the_masks_have_the_zeros_the_mutant_cases_count_on():
    for S in (33, 65, 160, 257):
        for mk in MASKED:
            m = K.make_mask(mk, ITEMS, S)
            assert (m[:, 32:] == 0).any().item(), (mk, S)            # a masked text key
            assert (m.sum(-1) > 0).any().item()
        assert not torch.equal(K.make_mask("ragged", ITEMS, S)[0], K.make_mask("ragged", ITEMS, S)[2])
    assert (K.make_mask("zero_row", ITEMS, 160)[1] == 0).all().item()


def test_debug_entry_refuses_bad_arguments_before_any_launch():
    """No device is touched: every call below returns MRA_EINVAL from the argument check."""
    L = _lib.lib()
    fake = 4096     # an aligned non-null address that is never dereferenced
    F16, BF16, F32 = _lib.MRA_F16, _lib.MRA_BF16, _lib.MRA_F32

    def call(qkv=fake, mask=None, ctx=fake, d_ctx=fake, lse=fake, dtype=F16, items=2, S=33, heads=2, dqkv=fake):
        return L.mra_debug_self_attention_bwd(qkv, mask, ctx, d_ctx, lse, dtype, items, S, heads, dqkv, None)

    for name in ("qkv", "ctx", "d_ctx", "lse", "dqkv"):
        assert call(**{name: None}) == -1 and b"null" in L.mra_last_error(), name
    for name in ("items", "S", "heads"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -1 and b"sizes" in L.mra_last_error(), (name, bad)
    assert call(dtype=F32) == -1 and b"dtype" in L.mra_last_error()
    assert call(qkv=fake + 2) == -1 and b"aligned" in L.mra_last_error()
    for dtype in (F16, BF16):
        assert call(dtype=dtype, S=SB.MAX_S + 1) == -1 and b"448" in L.mra_last_error()
        assert call(dtype=dtype, S=100000) == -1 and b"448" in L.mra_last_error()
