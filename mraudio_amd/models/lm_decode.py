"""The attached LM's decode: one-token attention on HIP over a K/V cache that is read in place.

The reference picks its best checkpoint by decoding the validation set with ``self.llm_model.generate(inputs_embeds=..., attention_mask=...)``
(``models/xinstructblip.py:383-391``, ``utils/trainer.py:157-165``).  Behind a prefix of a few thousand positions every new token reads the
whole K/V of every layer; the stock route (a ``DynamicCache`` whose ``update`` is a ``torch.cat``) also copies it.  Here:

    decode_attention(q, k, v, mask, scale)     out[b,h] = softmax_s(scale q[b,h] . k[b, h / G, s] over the attended s) v[b, h / G]
                                               logits, softmax and P V in fp32, one rounding; ``mra_decode_attention`` on the GPU (K / V as
                                               strided views: a static cache's buffer is never copied), the same definition as torch ops
                                               elsewhere -- the oracle of the tests
    register()                                 the function under the name "mra_decode" in transformers' ``AttentionInterface``: one-token
                                               calls of an evaluating module go to ``decode_attention``, everything else (the prefill above
                                               all) to transformers' own ``sdpa_attention_forward`` with the arguments untouched
    hip_decode(llm)                            context manager: the LM runs with that implementation inside the block and is as it was after it

A row with no attended key gives +0 where SDPA gives NaN; ``generate`` never produces one.  Out of scope: paged or quantised K/V, beam search
and sampling, a prefill kernel, sliding windows and soft caps (such calls go to SDPA)."""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

from .._lib import MraError, check, current_stream, lib, mra_dtype, ptr

NAME = "mra_decode"
HEAD_DIMS, GROUPS = (64, 128), (1, 2, 4, 8)


def _shapes(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor]) -> Optional[str]:
    """None when the tensors are a one-token attention call, else what is wrong."""
    if q.dim() != 4 or k.dim() != 4 or q.shape[2] != 1 or k.shape != v.shape or k.shape[0] != q.shape[0] or k.shape[3] != q.shape[3] or k.shape[2] < 1 \
            or k.shape[1] < 1 or q.shape[1] % k.shape[1]:
        return f"q [B, Hq, 1, D], k / v [B, Hkv, S, D] with Hq a multiple of Hkv expected, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}"
    if mask is not None and (mask.dtype != torch.bool or mask.dim() != 4 or tuple(mask.shape[1:]) != (1, 1, k.shape[2]) or mask.shape[0] not in (1, q.shape[0])):
        return f"mask must be bool [B, 1, 1, S] (True = attend) or None, got {mask.dtype} {tuple(mask.shape)}"
    return None


def accepted(q: torch.Tensor, k: torch.Tensor) -> bool:
    """The shapes ``mra_decode_attention`` takes: D 64 or 128, Hq / Hkv 1, 2, 4 or 8."""
    return q.shape[3] in HEAD_DIMS and q.shape[1] // k.shape[1] in GROUPS and q.shape[0] <= 65535 and k.shape[1] <= 65535


def _hip_reason(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor]) -> Optional[str]:
    """None when the HIP entry applies, else why not."""
    if not (q.is_cuda and k.is_cuda and v.is_cuda and (mask is None or mask.is_cuda)):
        return "q, k, v and the mask must be CUDA tensors"
    if not (q.dtype == k.dtype == v.dtype) or q.dtype not in (torch.float16, torch.bfloat16):
        return f"q, k and v must share a 16-bit dtype, got {q.dtype}, {k.dtype}, {v.dtype}"
    if not accepted(q, k):
        return f"D = {q.shape[3]} with Hq / Hkv = {q.shape[1] // k.shape[1]} is outside D in {HEAD_DIMS}, Hq / Hkv in {GROUPS}"
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.stride(3) != 1 or any(s % 8 for s in t.stride()[:3]) or t.data_ptr() % 16 or (name != "q" and t.stride(2) < t.shape[3]):
            return f"{name} is not laid out as the entry reads it (unit stride along D, 16-byte aligned rows), and no copy of it is made"
    return None


def _entry(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor], scale: float) -> torch.Tensor:
    B, Hq, _, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    out = torch.empty(B, Hq, 1, D, dtype=q.dtype, device=q.device)
    m8, m_sb = None, 0
    if mask is not None:
        m8 = (mask if mask.stride(3) == 1 or S == 1 else mask.contiguous()).view(torch.uint8)      # [B or 1, 1, 1, S] bytes: a few KB at most
        m_sb = m8.stride(0) if mask.shape[0] == B and B > 1 else 0
    nbytes = int(lib().mra_decode_attention_workspace_bytes(B, Hq, S, D))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
    check(lib().mra_decode_attention(ptr(q), q.stride(0), q.stride(1), ptr(k), k.stride(0), k.stride(1), k.stride(2), ptr(v), v.stride(0), v.stride(1),
                                     v.stride(2), None if m8 is None else ptr(m8), m_sb, B, Hq, Hkv, S, D, mra_dtype(q.dtype), float(scale), ptr(out),
                                     Hq * D, D, None, ptr(ws), nbytes, current_stream()), "mra_decode_attention")
    return out


def _torch_ops(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor], scale: float) -> torch.Tensor:
    """The definition in fp32 (wider inputs keep their type).  Masking is a select on both sides: a masked slot's bits reach nothing."""
    G = q.shape[1] // k.shape[1]
    ct = torch.float32 if q.dtype in (torch.float16, torch.bfloat16) else q.dtype
    kf, vf = k.to(ct).repeat_interleave(G, dim=1), v.to(ct).repeat_interleave(G, dim=1)       # [B, Hq, S, D]
    z = scale * (q.to(ct) @ kf.transpose(2, 3))                                               # [B, Hq, 1, S]
    if mask is not None:
        z = torch.where(mask, z, torch.full((), float("-inf"), dtype=ct, device=z.device))
        vf = torch.where(mask.transpose(2, 3), vf, torch.zeros((), dtype=ct, device=z.device))
    m = z.max(dim=3, keepdim=True).values
    m = torch.where(m > float("-inf"), m, torch.zeros_like(m))                                # a row with no attended key: every p is 0
    p = torch.exp(z - m)
    l = p.sum(dim=3, keepdim=True)
    out = (p @ vf) / torch.where(l > 0, l, torch.ones_like(l))
    return out.to(q.dtype)


def decode_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor], scale: float,
                     hip: Optional[bool] = None) -> torch.Tensor:
    """``q`` [B, Hq, 1, D], ``k`` / ``v`` [B, Hkv, S, D] (views with any batch / head / key strides), ``mask`` bool [B, 1, 1, S] with True =
    attend, or None: ``[B, Hq, 1, D]`` in q's dtype.  ``hip=None`` takes ``mra_decode_attention`` where it accepts the call (CUDA, one 16-bit
    dtype, D 64 or 128, Hq / Hkv 1, 2, 4 or 8, 16-byte aligned rows) and the torch ops otherwise; ``hip=True`` raises ``MraError`` naming the
    reason; ``hip=False`` is the torch ops."""
    bad = _shapes(q, k, v, mask)
    if bad is not None:
        raise ValueError(f"decode_attention: {bad}")
    if hip is None or hip:
        why = _hip_reason(q, k, v, mask)
        if why is None:
            return _entry(q, k, v, mask, scale)
        if hip:
            raise MraError(f"decode_attention(hip=True): {why}")
    return _torch_ops(q, k, v, mask, scale)


def attention_forward(module, query, key, value, attention_mask, dropout=0.0, scaling=None, **kw):
    """What ``register`` registers.  One query position, an evaluating module, no dropout, a bool mask (or none) over the keys and accepted
    shapes: ``decode_attention``; anything else: transformers' SDPA function with the arguments as they came."""
    if (query.dim() == 4 and query.shape[2] == 1 and not module.training and not dropout and kw.get("sliding_window") is None
            and kw.get("softcap") is None and _shapes(query, key, value, attention_mask) is None and accepted(query, key)):
        scale = float(scaling) if scaling is not None else query.shape[3] ** -0.5
        out = decode_attention(query, key, value, attention_mask, scale)                    # [B, Hq, 1, D]
        return out.transpose(1, 2).contiguous(), None
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kw)


def register() -> str:
    """Put ``attention_forward`` and SDPA's mask builder under ``"mra_decode"`` in transformers' registries.  Idempotent; returns the name."""
    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface, sdpa_mask

    if AttentionInterface._global_mapping.get(NAME) is not attention_forward:
        AttentionInterface.register(NAME, attention_forward)
    if AttentionMaskInterface._global_mapping.get(NAME) is not sdpa_mask:
        AttentionMaskInterface.register(NAME, sdpa_mask)
    return NAME


@contextlib.contextmanager
def hip_decode(llm):
    """Run ``llm`` with the registered attention inside the block; its ``config._attn_implementation`` is put back on the way out, also after
    an exception.  Nothing else of the LM is touched."""
    prev = llm.config._attn_implementation
    llm.set_attn_implementation(register())
    try:
        yield llm
    finally:
        llm.set_attn_implementation(prev)
