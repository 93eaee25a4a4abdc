"""The attached LM's attention in training: the causal grouped-query attention as ONE autograd node on HIP.

The one regime the reference trains in (``finetune --lora --freeze-qformers --objective llm``) runs ``self.llm_model(inputs_embeds=...,
labels=...)`` (``models/xinstructblip.py:599-604``): in every layer transformers hands SDPA a bool ``[B, 1, S, S]`` mask, forward and backward.
Here:

    causal_attention(q, k, v, key_mask, scale, q_offset=0)
                                               the definition of ``lm_decode.prefill_attention``, differentiable.  On the GPU the forward is
                                               ``mra_prefill_attention`` with its ``lse``; q, k, v, out and lse are saved (no [Sq, Skv]
                                               tensor in either direction) and the backward is one ``mra_prefill_attention_backward``.
                                               Elsewhere: ``lm_decode._torch_ops`` under torch.autograd -- the oracle of the tests
    register_train(), hip_train(llm)           a third name, "mra_train", in transformers' ``AttentionInterface`` / ``AttentionMaskInterface``
                                               with ``lm_decode.prefill_mask`` as its mask builder: key-mask calls with no dropout, no sliding
                                               window, no soft cap and accepted shapes go to ``causal_attention`` whatever ``module.training``
                                               says (the reference trains with attention dropout 0; the adapters' dropout sits in
                                               ``LoraLinear``), everything else to ``lm_decode.prefill_attention_forward`` unchanged

    hold_for_backward(llm, loss)               activation checkpointing: the recomputation inside the backward runs the same attention

A query row with no attended key (a left-pad row) gives +0 and takes and gives no gradient.  Out of scope: attention dropout, sliding windows
and soft caps (such calls go to SDPA), the LM's linears, norms and rotary."""
from __future__ import annotations

import contextlib
import warnings
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from .._lib import MraError, check, current_stream, lib, mra_dtype, ptr
from . import lm_decode as _ld

TRAIN_NAME = "mra_train"


def _backward_entry(q, k, v, mask, out, dout, lse, scale: float, q_offset: int):
    """``mra_prefill_attention_backward``: (dq [B, Hq, Sq, D] as the transposed view of a [B, Sq, Hq, D] tensor, dk, dv [B, Hkv, Skv, D])."""
    B, Hq, Sq, D = q.shape
    Hkv, Skv = k.shape[1], k.shape[2]
    m8, m_sb = _ld._mask_bytes(mask, B)
    if dout.stride(3) != 1 or any(s % 8 for s in dout.stride()[:3]) or dout.data_ptr() % 16 or dout.stride(1) < D or dout.stride(2) < D:
        dout = dout.contiguous()
    dq = torch.empty(B, Sq, Hq, D, dtype=q.dtype, device=q.device).transpose(1, 2)
    dk, dv = torch.empty_like(k, memory_format=torch.contiguous_format), torch.empty_like(v, memory_format=torch.contiguous_format)
    nbytes = int(lib().mra_prefill_attention_backward_workspace_bytes(B, Hq, Sq))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=q.device)
    check(lib().mra_prefill_attention_backward(
        ptr(q), q.stride(0), q.stride(1), q.stride(2), ptr(k), k.stride(0), k.stride(1), k.stride(2), ptr(v), v.stride(0), v.stride(1), v.stride(2),
        None if m8 is None else ptr(m8), m_sb, ptr(out), out.stride(0), out.stride(1), out.stride(2), ptr(dout), dout.stride(0), dout.stride(1),
        dout.stride(2), ptr(lse), B, Hq, Hkv, Sq, Skv, int(q_offset), D, mra_dtype(q.dtype), float(scale), ptr(dq), dq.stride(0), dq.stride(1),
        dq.stride(2), ptr(dk), dk.stride(0), dk.stride(1), dk.stride(2), ptr(dv), dv.stride(0), dv.stride(1), dv.stride(2), ptr(ws), nbytes,
        current_stream()), "mra_prefill_attention_backward")
    return dq, dk, dv


class _CausalAttention(torch.autograd.Function):
    """out [B, Sq, Hq, D] = mra_prefill_attention(q, k, v); saves q, k, v, out and lse; one mra_prefill_attention_backward."""

    @staticmethod
    def forward(ctx, q, k, v, key_mask, scale, q_offset):
        out, lse = _ld._entry(q, k, v, key_mask, scale, q_offset, True)
        ctx.save_for_backward(q, k, v, out, lse, key_mask)                # the mask too: a change in place before the backward is an error
        ctx.scale, ctx.q_offset = scale, q_offset
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, out, lse, key_mask = ctx.saved_tensors
        dq, dk, dv = _backward_entry(q, k, v, key_mask, out, dout, lse, ctx.scale, ctx.q_offset)
        return dq, dk, dv, None, None, None


_warned = set()


def _warn_once(text: str) -> None:
    if text not in _warned:
        _warned.add(text)
        warnings.warn(text, RuntimeWarning, stacklevel=3)


def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, key_mask: Optional[torch.Tensor], scale: float, q_offset: int = 0,
                     hip: Optional[bool] = None) -> torch.Tensor:
    """``lm_decode.prefill_attention`` with a gradient: ``q`` [B, Hq, Sq, D], ``k`` / ``v`` [B, Hkv, Skv, D], ``key_mask`` bool [B, 1, 1, Skv]
    (True = attend) or None, query row i at key slot ``q_offset + i``: ``[B, Sq, Hq, D]`` in q's dtype.  Where ``mra_prefill_attention``
    accepts the call it is one autograd node whose backward is ``mra_prefill_attention_backward``; ``hip=False``, CPU tensors or a call the
    entry does not take run ``lm_decode._torch_ops`` under torch.autograd; ``hip=True`` raises ``MraError`` naming the reason.  Under
    ``no_grad``, or when no input requires a gradient, it is ``prefill_attention``, bit for bit."""
    if not (torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)):
        return _ld.prefill_attention(q, k, v, key_mask, scale, q_offset=q_offset, hip=hip)
    bad = _ld._shapes(q, k, v, key_mask, int(q_offset))
    if bad is not None:
        raise ValueError(f"causal_attention: {bad}")
    if hip is None or hip:
        why = _ld._hip_reason(q, k, v, key_mask, False)
        if why is None:
            return _CausalAttention.apply(q, k, v, key_mask, float(scale), int(q_offset))
        if hip:
            raise MraError(f"causal_attention(hip=True): {why}")
        if q.is_cuda:
            _warn_once(f"causal_attention: the torch ops take this call on the GPU, with an fp32 [B, Hq, Sq, Skv] tensor in both directions: {why}")
    out, _ = _ld._torch_ops(q, k, v, key_mask, scale, int(q_offset))
    return out.transpose(1, 2).contiguous()


def train_attention_forward(module, query, key, value, attention_mask, dropout=0.0, scaling=None, **kw):
    """What ``register_train`` registers.  More than one query row under the key mask of ``prefill_mask`` (q_offset 0), no dropout, no sliding
    window or soft cap and accepted shapes, in training or not: ``causal_attention``.  Everything else is ``prefill_attention_forward``."""
    if _ld._is_key_mask(query, key, attention_mask) and not dropout and kw.get("sliding_window") is None and kw.get("softcap") is None \
            and _ld._shapes(query, key, value, attention_mask, 0) is None and _ld.accepted(query, key):
        scale = float(scaling) if scaling is not None else query.shape[3] ** -0.5
        return causal_attention(query, key, value, attention_mask, scale, q_offset=0), None        # [B, Sq, Hq, D] as it is wanted back
    return _ld.prefill_attention_forward(module, query, key, value, attention_mask, dropout=dropout, scaling=scaling, **kw)


def register_train() -> str:
    """Put ``train_attention_forward`` and ``lm_decode.prefill_mask`` under ``"mra_train"`` in transformers' registries.  Idempotent."""
    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface

    if AttentionInterface._global_mapping.get(TRAIN_NAME) is not train_attention_forward:
        AttentionInterface.register(TRAIN_NAME, train_attention_forward)
    if AttentionMaskInterface._global_mapping.get(TRAIN_NAME) is not _ld.prefill_mask:
        AttentionMaskInterface.register(TRAIN_NAME, _ld.prefill_mask)
    return TRAIN_NAME


class _HoldForBackward(torch.autograd.Function):
    """Identity on the loss.  Its backward runs first of the whole pass: it puts the training attention back in force, so that the layers an
    activation checkpoint recomputes run what the forward ran (their saved mask is the key mask alone, which only this implementation
    reads as causal), and queues the way back for the end of the pass."""

    @staticmethod
    def forward(ctx, loss, llm):
        ctx.llm = llm
        return loss.view_as(loss)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        llm = ctx.llm
        prev = llm.config._attn_implementation
        if prev != TRAIN_NAME:
            llm.set_attn_implementation(register_train())
            torch.autograd.Variable._execution_engine.queue_callback(lambda: llm.set_attn_implementation(prev))
        return grad, None


def hold_for_backward(llm, loss: torch.Tensor) -> torch.Tensor:
    """``loss`` of a forward made inside ``hip_train(llm)``, for an LM with activation checkpointing: the same value, whose backward runs
    the recomputation under the training attention and leaves ``config._attn_implementation`` as it found it when the pass ends.  An LM
    without checkpointing, or a loss that needs no gradient, gets ``loss`` back untouched."""
    if not (getattr(llm, "is_gradient_checkpointing", False) and loss.requires_grad):
        return loss
    return _HoldForBackward.apply(loss, llm)


@contextlib.contextmanager
def hip_train(llm):
    """Run ``llm`` with the training attention inside the block; its ``config._attn_implementation`` is put back on the way out, also after
    an exception.  Nothing else of the LM is touched.  With activation checkpointing the backward recomputes layers after the block: pass
    the loss through ``hold_for_backward`` (``XInstructBLIP._lm_ce`` does)."""
    prev = llm.config._attn_implementation
    llm.set_attn_implementation(register_train())
    try:
        yield llm
    finally:
        llm.set_attn_implementation(prev)
