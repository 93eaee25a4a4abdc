"""Two things the LM routes have ONE of, without a GPU (``-m "not gpu"``).

The torch definition of the masked softmax in ``mraudio_amd/models/lm_decode.py``: the oracle of the decode, prefill and step tests.  It
replaced two functions (one per route); tests/golden/lm_attention_parent.npz holds what those two returned in float64 on rows of the two case
tables (the operands of ``make_case`` in float16, widened), and the definition must return the same bits -- an oracle that moves would move
every bound measured against it.  The one-token call is the causal call with one row at the last slot, bit for bit.

``check_lm_options`` of ``mraudio_amd/models/xinstructblip.py``: the one rule for the pair (lm_decode, lm_prefill)."""
import os

import numpy as np
import pytest
import torch

import decode_attn_cases as DC
import prefill_attn_cases as PC
from mraudio_amd import _lib
from mraudio_amd.models import lm_decode as LD
from mraudio_amd.models.xinstructblip import LM_DECODES, LM_PREFILLS, check_lm_options, check_lm_prefill

B_DECODE, B_PREFILL, D = 3, 2, 64
DECODE_ROWS = [(S, mask, Hq, Hkv) for S in (1, 65, 257) for mask in ("holes", "row_masked") for Hq, Hkv in ((8, 2), (3, 3))]
PREFILL_ROWS = [(Sq, Skv, off, mask) for Sq, Skv, off in ((1, 1, 0), (33, 33, 0), (5, 40, 35)) for mask in ("holes", "row_masked")]


@pytest.fixture(scope="module")
def parent(golden_dir):
    with np.load(os.path.join(golden_dir, "lm_attention_parent.npz")) as z:
        return {k: torch.from_numpy(z[k]) for k in z.files}


def _decode_case(S, mask, Hq, Hkv):
    c = DC.make_case(B_DECODE, Hq, Hkv, S, D, mask, torch.float16)
    return c["q"].double()[:, :, None], c["k"].double(), c["v"].double(), c["mask"][:, None, None, :], c["scale"]


@pytest.mark.parametrize("S,mask,Hq,Hkv", DECODE_ROWS)
def test_decode_route_returns_the_parents_bits_and_is_the_last_row_of_the_prefill_route(parent, S, mask, Hq, Hkv):
    q, k, v, m, scale = _decode_case(S, mask, Hq, Hkv)
    out = LD.decode_attention(q, k, v, m, scale, hip=False)
    assert out.dtype == torch.float64 and tuple(out.shape) == (B_DECODE, Hq, 1, D)
    assert torch.equal(out, parent[f"decode_S{S}_{mask}_{Hq}x{Hkv}"])
    pre, lse = LD.prefill_attention(q, k, v, m, scale, q_offset=S - 1, hip=False, want_lse=True)          # [B, 1, Hq, D]
    assert torch.equal(out, pre.transpose(1, 2))
    if mask == "row_masked":                                   # the last batch row attends nothing: +0 and -inf, not NaN
        assert not out[-1].any() and not torch.signbit(out[-1]).any() and bool((lse[-1] == float("-inf")).all())
    for dt in (torch.float16, torch.bfloat16):                 # the 16-bit routes agree the same way
        q16, k16, v16 = q.to(dt), k.to(dt), v.to(dt)
        assert torch.equal(LD.decode_attention(q16, k16, v16, m, scale, hip=False),
                           LD.prefill_attention(q16, k16, v16, m, scale, q_offset=S - 1, hip=False).transpose(1, 2))


@pytest.mark.parametrize("Sq,Skv,off,mask", PREFILL_ROWS)
def test_prefill_route_returns_the_parents_bits(parent, Sq, Skv, off, mask):
    c = PC.make_case(B_PREFILL, 4, 2, Sq, Skv, off, D, mask, torch.float16)
    out, lse = LD.prefill_attention(c["q"].double(), c["k"].double(), c["v"].double(), c["mask"][:, None, None, :], c["scale"], q_offset=off, hip=False,
                                    want_lse=True)
    assert out.dtype == torch.float64 and tuple(out.shape) == (B_PREFILL, Sq, 4, D) and out.is_contiguous()
    assert torch.equal(out, parent[f"prefill_{Sq}_{Skv}_{off}_{mask}"])
    assert torch.equal(lse, parent[f"prefill_{Sq}_{Skv}_{off}_{mask}_lse"])


# ---- the option check -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lm_prefill", LM_PREFILLS)
@pytest.mark.parametrize("lm_decode", LM_DECODES)
def test_check_lm_options_over_the_grid(lm_decode, lm_prefill):
    assert LM_DECODES == ("stock", "hip", "hip_step") and LM_PREFILLS == ("stock", "hip")
    if lm_prefill == "hip" and lm_decode == "stock":
        for call in (lambda: check_lm_options(lm_decode, lm_prefill), lambda: check_lm_prefill(lm_prefill, lm_decode),
                     lambda: check_lm_options(lm_decode, lm_prefill, unknown_decode=_lib.MraError)):
            with pytest.raises(ValueError, match="lm_prefill='hip' needs lm_decode 'hip' or 'hip_step'"):
                call()
    else:
        assert check_lm_options(lm_decode, lm_prefill) is None and check_lm_prefill(lm_prefill, lm_decode) is None


def test_check_lm_options_refuses_an_unknown_value_of_either():
    with pytest.raises(ValueError, match="lm_decode must be 'stock', 'hip' or 'hip_step', got 'fast'"):
        check_lm_options("fast")
    with pytest.raises(_lib.MraError, match="lm_decode must be 'stock', 'hip' or 'hip_step', got 'fast'"):      # _llm_decode's type
        check_lm_options("fast", "stock", unknown_decode=_lib.MraError)
    for lm_decode in LM_DECODES:
        with pytest.raises(ValueError, match="lm_prefill must be 'stock' or 'hip', got 'bogus'"):
            check_lm_options(lm_decode, "bogus")
