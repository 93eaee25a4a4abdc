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

The prefill in front of it (the reference's same ``generate`` call, ``models/xinstructblip.py:388-391``) is opt-in:

    prefill_attention(q, k, v, key_mask, scale, q_offset=0)
                                               out[b,i,h] = softmax over {s <= q_offset + i, key_mask[b,s]} of scale q[b,h,i] . k[b, h / G, s],
                                               times v: causality and the key mask are applied inside, the HIP route has no [Sq, Skv] tensor;
                                               ``mra_prefill_attention`` on the GPU, the same definition as torch ops elsewhere
    register(prefill=True), hip_decode(llm, prefill=True)
                                               a second name, "mra_prefill": its mask builder hands the FIRST prefill (q_offset 0, more than
                                               one query, the plain causal mask function) the key mask alone, bool [B, 1, 1, kv_length]; its
                                               attention function sends such calls to ``prefill_attention``, one-token calls to
                                               ``decode_attention`` and everything else to SDPA (under the full causal mask, rebuilt if the
                                               call carried the key mask alone)

A row with no attended key gives +0 where SDPA gives NaN; ``generate`` never produces one behind a decode, and the left-pad query rows of a
prefill, which are exactly that case, are attended by nothing downstream.  Out of scope: paged or quantised K/V, beam search and sampling,
chunked prefill, sliding windows and soft caps (such calls go to SDPA)."""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

from .._lib import MraError, check, current_stream, lib, mra_dtype, ptr

NAME = "mra_decode"
PREFILL_NAME = "mra_prefill"
HEAD_DIMS, GROUPS = (64, 128), (1, 2, 4, 8)


def _shapes(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor], q_offset: Optional[int] = None) -> Optional[str]:
    """None when the tensors are an attention call, else what is wrong.  ``q_offset`` None: the one-token call (one query row, which sits
    at the last key slot); an int: the causal call of Sq rows, row i at key slot ``q_offset + i``."""
    one = q_offset is None
    sq, skv, mname = ("1", "S", "mask") if one else ("Sq", "Skv", "key_mask")
    if q.dim() != 4 or k.dim() != 4 or (q.shape[2] != 1 if one else q.shape[2] < 1) or k.shape != v.shape or k.shape[0] != q.shape[0] \
            or k.shape[3] != q.shape[3] or k.shape[2] < 1 or k.shape[1] < 1 or q.shape[1] % k.shape[1]:
        return f"q [B, Hq, {sq}, D], k / v [B, Hkv, {skv}, D] with Hq a multiple of Hkv expected, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}"
    if not one and (q_offset < 0 or q_offset + q.shape[2] > k.shape[2]):
        return f"0 <= q_offset and q_offset + Sq <= Skv expected, got q_offset {q_offset}, Sq {q.shape[2]}, Skv {k.shape[2]}"
    if mask is not None and (mask.dtype != torch.bool or mask.dim() != 4 or tuple(mask.shape[1:]) != (1, 1, k.shape[2]) or mask.shape[0] not in (1, q.shape[0])):
        return f"{mname} must be bool [B, 1, 1, {skv}] (True = attend) or None, got {mask.dtype} {tuple(mask.shape)}"
    return None


def accepted(q: torch.Tensor, k: torch.Tensor) -> bool:
    """The shapes ``mra_decode_attention`` takes: D 64 or 128, Hq / Hkv 1, 2, 4 or 8."""
    return q.shape[3] in HEAD_DIMS and q.shape[1] // k.shape[1] in GROUPS and q.shape[0] <= 65535 and k.shape[1] <= 65535


def _hip_reason(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor], one: bool) -> Optional[str]:
    """None when the HIP entry applies (``one``: ``mra_decode_attention``, else ``mra_prefill_attention``), else why not."""
    if not (q.is_cuda and k.is_cuda and v.is_cuda and (mask is None or mask.is_cuda)):
        return f"q, k, v and the {'mask' if one else 'key mask'} must be CUDA tensors"
    if not (q.dtype == k.dtype == v.dtype) or q.dtype not in (torch.float16, torch.bfloat16):
        return f"q, k and v must share a 16-bit dtype, got {q.dtype}, {k.dtype}, {v.dtype}"
    if not accepted(q, k):
        return f"D = {q.shape[3]} with Hq / Hkv = {q.shape[1] // k.shape[1]} is outside D in {HEAD_DIMS}, Hq / Hkv in {GROUPS}"
    if not one and (k.shape[2] > 1 << 30 or q.shape[2] > 65535 * 256):
        return f"Sq = {q.shape[2]}, Skv = {k.shape[2]} is outside the entry's grid"
    for name, t in (("q", q), ("k", k), ("v", v)):                   # the one query row of a decode has no position stride to speak of
        if t.stride(3) != 1 or any(s % 8 for s in t.stride()[:3]) or t.data_ptr() % 16 or (not (one and name == "q") and t.stride(2) < t.shape[3]):
            return f"{name} is not laid out as the entry reads it (unit stride along D, 16-byte aligned rows), and no copy of it is made"
    return None


def _mask_bytes(mask: Optional[torch.Tensor], B: int):
    """``(bytes, batch stride)`` of the mask as the entries read it, uint8 [B or 1, 1, 1, S] (a copy of a few KB at most, which the caller
    keeps until its launch is enqueued); (None, 0) without one."""
    if mask is None:
        return None, 0
    m8 = (mask if mask.stride(3) == 1 or mask.shape[3] == 1 else mask.contiguous()).view(torch.uint8)
    return m8, m8.stride(0) if mask.shape[0] == B and B > 1 else 0


def _entry(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor], scale: float, q_offset: Optional[int], want_lse: bool):
    """The HIP entries: ``(out, lse)`` with out [B, Hq, 1, D] and no lse for the one-token call, out [B, Sq, Hq, D] for the causal one."""
    B, Hq, Sq, D = q.shape
    Hkv, S = k.shape[1], k.shape[2]
    m8, m_sb = _mask_bytes(mask, B)
    mp = None if m8 is None else ptr(m8)
    if q_offset is None:
        out = torch.empty(B, Hq, 1, D, dtype=q.dtype, device=q.device)
        nbytes = int(lib().mra_decode_attention_workspace_bytes(B, Hq, S, D))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
        check(lib().mra_decode_attention(ptr(q), q.stride(0), q.stride(1), ptr(k), k.stride(0), k.stride(1), k.stride(2), ptr(v), v.stride(0), v.stride(1),
                                         v.stride(2), mp, m_sb, B, Hq, Hkv, S, D, mra_dtype(q.dtype), float(scale), ptr(out), Hq * D, D, None, ptr(ws),
                                         nbytes, current_stream()), "mra_decode_attention")
        return out, None
    out = torch.empty(B, Sq, Hq, D, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, Hq, Sq, dtype=torch.float32, device=q.device) if want_lse else None
    check(lib().mra_prefill_attention(ptr(q), q.stride(0), q.stride(1), q.stride(2), ptr(k), k.stride(0), k.stride(1), k.stride(2), ptr(v), v.stride(0),
                                      v.stride(1), v.stride(2), mp, m_sb, B, Hq, Hkv, Sq, S, q_offset, D, mra_dtype(q.dtype), float(scale), ptr(out),
                                      out.stride(0), out.stride(1), out.stride(2), None if lse is None else ptr(lse), current_stream()),
          "mra_prefill_attention")
    return out, lse


def _torch_ops(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor], scale: float, q_offset: int):
    """THE definition, in fp32 (wider inputs keep their type): ``(out [B, Hq, Sq, D] in q's dtype, lse [B, Hq, Sq])`` of query rows i at key
    slots ``q_offset + i`` over the keys s <= q_offset + i that the mask lets through.  The one-token call is Sq = 1, q_offset = S - 1.
    Masking is a select on both sides: the bits of a key that no row attends reach nothing."""
    Hq, Sq = q.shape[1], q.shape[2]
    Skv = k.shape[2]
    G = Hq // k.shape[1]
    ct = torch.float32 if q.dtype in (torch.float16, torch.bfloat16) else q.dtype
    dev = q.device
    on = torch.arange(Skv, device=dev)[None, :] <= (torch.arange(Sq, device=dev) + q_offset)[:, None]     # [Sq, Skv]: a few MB at the tests' sizes
    on = on[None, None] if mask is None else on[None, None] & mask.to(dev)                              # [B or 1, 1, Sq, Skv]
    some = on.any(dim=2)[..., None]                                                                     # [B or 1, 1, Skv, 1]: attended by a row
    zero = torch.zeros((), dtype=ct, device=dev)
    kf = torch.where(some, k.to(ct), zero).repeat_interleave(G, dim=1)                                        # [B, Hq, Skv, D]
    vf = torch.where(some, v.to(ct), zero).repeat_interleave(G, dim=1)
    z = torch.where(on, scale * (q.to(ct) @ kf.transpose(2, 3)), torch.full((), float("-inf"), dtype=ct, device=dev))   # [B, Hq, Sq, Skv]
    m = z.max(dim=3, keepdim=True).values
    live = m > float("-inf")
    m = torch.where(live, m, torch.zeros_like(m))                                                             # a row with no attended key: every p is 0
    p = torch.exp(z - m)
    l = p.sum(dim=3, keepdim=True)
    l1 = torch.where(live, l, torch.ones_like(l))
    lse = torch.where(live, m + torch.log(l1), torch.full((), float("-inf"), dtype=ct, device=dev))[..., 0]
    return ((p @ vf) / l1).to(q.dtype), lse


def _attention(name: str, q, k, v, mask, scale: float, q_offset: Optional[int], hip: Optional[bool], want_lse: bool = False):
    """``(out, lse)`` of ``decode_attention`` (``q_offset`` None) / ``prefill_attention``, each in its own output layout: the HIP entry where
    ``hip`` allows it and it applies, ``MraError`` naming the reason under ``hip=True``, the torch ops otherwise."""
    bad = _shapes(q, k, v, mask, q_offset)
    if bad is not None:
        raise ValueError(f"{name}: {bad}")
    if hip is None or hip:
        why = _hip_reason(q, k, v, mask, q_offset is None)
        if why is None:
            return _entry(q, k, v, mask, scale, q_offset, want_lse)
        if hip:
            raise MraError(f"{name}(hip=True): {why}")
    if q_offset is None:
        return _torch_ops(q, k, v, mask, scale, k.shape[2] - 1)
    out, lse = _torch_ops(q, k, v, mask, scale, q_offset)
    return out.transpose(1, 2).contiguous(), lse


def decode_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: Optional[torch.Tensor], scale: float,
                     hip: Optional[bool] = None) -> torch.Tensor:
    """``q`` [B, Hq, 1, D], ``k`` / ``v`` [B, Hkv, S, D] (views with any batch / head / key strides), ``mask`` bool [B, 1, 1, S] with True =
    attend, or None: ``[B, Hq, 1, D]`` in q's dtype.  ``hip=None`` takes ``mra_decode_attention`` where it accepts the call (CUDA, one 16-bit
    dtype, D 64 or 128, Hq / Hkv 1, 2, 4 or 8, 16-byte aligned rows) and the torch ops otherwise; ``hip=True`` raises ``MraError`` naming the
    reason; ``hip=False`` is the torch ops."""
    return _attention("decode_attention", q, k, v, mask, scale, None, hip)[0]


def prefill_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_mask: Optional[torch.Tensor], scale: float, q_offset: int = 0,
                      hip: Optional[bool] = None, want_lse: bool = False):
    """``q`` [B, Hq, Sq, D], ``k`` / ``v`` [B, Hkv, Skv, D] (views with any batch / head / position strides), ``key_mask`` bool [B, 1, 1, Skv]
    with True = attend, or None; query row i sits at key slot ``q_offset + i`` and attends the keys s <= q_offset + i that the mask lets
    through: ``[B, Sq, Hq, D]`` in q's dtype (the layout transformers wants back), with ``want_lse`` the pair (out, lse fp32 [B, Hq, Sq]).
    ``hip=None`` takes ``mra_prefill_attention`` where it accepts the call (CUDA, one 16-bit dtype, D 64 or 128, Hq / Hkv 1, 2, 4 or 8,
    16-byte aligned rows) and the torch ops otherwise; ``hip=True`` raises ``MraError`` naming the reason; ``hip=False`` is the torch ops."""
    out, lse = _attention("prefill_attention", q, k, v, key_mask, scale, int(q_offset), hip, want_lse)
    return (out, lse) if want_lse else out


def _plain_scale(module, query, key, value, mask, dropout, scaling, kw, q_offset: Optional[int]) -> Optional[float]:
    """The scale of a call the two routes define -- an evaluating module, no dropout, no sliding window, no soft cap, a bool mask (or none)
    over the keys and accepted shapes -- and None for every other call, which is SDPA's."""
    if module.training or dropout or kw.get("sliding_window") is not None or kw.get("softcap") is not None \
            or _shapes(query, key, value, mask, q_offset) is not None or not accepted(query, key):
        return None
    return float(scaling) if scaling is not None else query.shape[3] ** -0.5


def _is_key_mask(query: torch.Tensor, key: torch.Tensor, attention_mask) -> bool:
    """The mask ``prefill_mask`` hands a first prefill: bool [B, 1, 1, Skv] under more than one query row."""
    return (isinstance(attention_mask, torch.Tensor) and attention_mask.dtype == torch.bool and query.dim() == 4 and query.shape[2] > 1
            and attention_mask.dim() == 4 and tuple(attention_mask.shape[1:]) == (1, 1, key.shape[2]) and attention_mask.shape[0] in (1, query.shape[0]))


def prefill_attention_forward(module, query, key, value, attention_mask, dropout=0.0, scaling=None, **kw):
    """What ``register(prefill=True)`` registers.  More than one query row under the key mask of ``prefill_mask`` (q_offset 0), an evaluating
    module, no dropout, no sliding window or soft cap and accepted shapes: ``prefill_attention``.  Such a call that is not accepted goes to
    SDPA under the full causal mask, built here from the key mask.  Everything else is ``attention_forward``."""
    if not _is_key_mask(query, key, attention_mask):
        return attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kw)
    scale = _plain_scale(module, query, key, value, attention_mask, dropout, scaling, kw, 0)
    if scale is not None:
        return prefill_attention(query, key, value, attention_mask, scale, q_offset=0), None       # [B, Sq, Hq, D] as it is wanted back
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    Sq, Skv, dev = query.shape[2], key.shape[2], query.device
    causal = torch.arange(Skv, device=dev)[None, :] <= torch.arange(Sq, device=dev)[:, None]
    full = (attention_mask & causal[None, None]).expand(query.shape[0], 1, Sq, Skv)                 # never silently non-causal
    return sdpa_attention_forward(module, query, key, value, full, dropout=dropout, scaling=scaling, **kw)


def prefill_mask(batch_size, q_length, kv_length, q_offset=0, kv_offset=0, mask_function=None, attention_mask=None, **kw):
    """The mask builder under ``"mra_prefill"``.  A first prefill (q_offset 0, kv_offset 0, more than one query row, the plain causal mask
    function, a 2-D padding mask or none): the key mask alone, bool [B, 1, 1, kv_length] (ones without a padding mask; False behind the
    padding mask's end, which is the unwritten tail of a static cache).  Everything else: ``sdpa_mask`` with the arguments as they came."""
    from transformers.masking_utils import causal_mask_function, prepare_padding_mask, sdpa_mask

    if mask_function is None:
        mask_function = causal_mask_function
    first = (mask_function is causal_mask_function and int(q_length) > 1 and int(kv_offset) == 0 and int(q_offset) == 0 and int(kv_length) >= int(q_length)
             and kw.get("local_size") is None and (attention_mask is None or attention_mask.dim() == 2))
    if not first:
        return sdpa_mask(batch_size=batch_size, q_length=q_length, kv_length=kv_length, q_offset=q_offset, kv_offset=kv_offset,
                         mask_function=mask_function, attention_mask=attention_mask, **kw)
    pad = prepare_padding_mask(attention_mask, kv_length, kv_offset)
    if pad is None:
        return torch.ones(batch_size, 1, 1, kv_length, dtype=torch.bool, device=kw.get("device", "cpu"))
    return pad[:, :kv_length].to(torch.bool)[:, None, None, :]


def attention_forward(module, query, key, value, attention_mask, dropout=0.0, scaling=None, **kw):
    """What ``register`` registers.  One query position, an evaluating module, no dropout, a bool mask (or none) over the keys and accepted
    shapes: ``decode_attention``; anything else: transformers' SDPA function with the arguments as they came."""
    scale = _plain_scale(module, query, key, value, attention_mask, dropout, scaling, kw, None)
    if scale is not None:
        return decode_attention(query, key, value, attention_mask, scale).transpose(1, 2).contiguous(), None      # [B, Hq, 1, D] -> [B, 1, Hq, D]
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    return sdpa_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kw)


def register(prefill: bool = False) -> str:
    """Put ``attention_forward`` and SDPA's mask builder under ``"mra_decode"`` in transformers' registries; with ``prefill``,
    ``prefill_attention_forward`` and ``prefill_mask`` under ``"mra_prefill"`` instead.  Idempotent; returns the name."""
    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface, sdpa_mask

    name, fn, mask = (PREFILL_NAME, prefill_attention_forward, prefill_mask) if prefill else (NAME, attention_forward, sdpa_mask)
    if AttentionInterface._global_mapping.get(name) is not fn:
        AttentionInterface.register(name, fn)
    if AttentionMaskInterface._global_mapping.get(name) is not mask:
        AttentionMaskInterface.register(name, mask)
    return name


@contextlib.contextmanager
def hip_decode(llm, prefill: bool = False):
    """Run ``llm`` with the registered attention inside the block (``prefill``: the one that also takes the first prefill); its
    ``config._attn_implementation`` is put back on the way out, also after an exception.  Nothing else of the LM is touched."""
    prev = llm.config._attn_implementation
    llm.set_attn_implementation(register(prefill))
    try:
        yield llm
    finally:
        llm.set_attn_implementation(prev)
