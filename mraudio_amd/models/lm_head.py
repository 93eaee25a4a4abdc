"""The LM objective's vocabulary head and cross-entropy on the labelled rows only.

The reference computes its loss with ``self.llm_model(inputs_embeds=..., attention_mask=..., return_dict=True, labels=targets)``
(``models/xinstructblip.py:599-604``): ``lm_head`` over every position, the logits upcast to fp32 (transformers' ``ForCausalLMLoss``), and a
cross-entropy that ignores every row whose label is -100 -- about 98 % of them.  ``lm_head_ce`` is the same definition on the rows that count:

    position t predicts labels[t + 1] (the causal shift of ForCausalLMLoss); the rows with a label other than -100 are gathered
    z = h_rows W^T in fp32, never rounded to 16 bits;  lse_r = log sum_v exp z_rv;  nll_r = lse_r - z_r,y_r;  loss = mean_r nll_r
    d h_rows = g_r (softmax(z_r) - e_y_r) W,  g_r = d loss / n

No ``[B, S, V]`` tensor exists in either direction.  On the GPU with a 16-bit LM the rows go through the HIP entries ``mra_lm_head_ce_forward`` /
``mra_lm_head_ce_backward`` as ONE autograd node (2 launches forward, 2 backward, ``W`` read as stored, no atomics); on the CPU, or with
``hip=False``, the same definition runs as torch ops under torch.autograd -- the oracle of the tests and the ``"rows"`` route.  The stock
route rounds its logits to the LM's dtype before the upcast; this one does not, so the two differ by that rounding.

``weight`` gets a gradient on the torch route only: the HIP route has no dW (the reference never trains ``lm_head``).  Out of scope: label
smoothing, z-loss, ``num_items_in_batch``, a bias on the head."""
from __future__ import annotations

from typing import Optional

import torch

from .._lib import MraError, check, current_stream, lib, mra_dtype, ptr

IGNORE = -100


def _hip_reason(hidden: torch.Tensor, weight: torch.Tensor) -> Optional[str]:
    """None when the HIP entries apply, else why not."""
    if not (hidden.is_cuda and weight.is_cuda):
        return "hidden and weight must be CUDA tensors"
    if hidden.dtype != weight.dtype or hidden.dtype not in (torch.float16, torch.bfloat16):
        return f"hidden and weight must share a 16-bit dtype, got {hidden.dtype} and {weight.dtype}"
    if hidden.shape[-1] % 8:
        return f"K = {hidden.shape[-1]} is not a multiple of 8"
    if weight.requires_grad and torch.is_grad_enabled():
        return "weight requires a gradient, which only the torch route computes"
    if weight.stride(1) != 1 or weight.stride(0) % 8 or weight.stride(0) < weight.shape[1] or weight.data_ptr() % 16:
        return "weight is not laid out as the entries read it (unit column stride, 16-byte aligned rows), and no copy of it is made"
    return None


def _forward_entries(rows: torch.Tensor, weight: torch.Tensor, y32: torch.Tensor, want_grad: bool):
    R, K = rows.shape
    V = weight.shape[0]
    dt = mra_dtype(rows.dtype)
    nbytes = int(lib().mra_lm_head_ce_workspace_bytes(R, V, K, dt, int(want_grad)))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=rows.device)
    nll = torch.empty(R, dtype=torch.float32, device=rows.device)
    lse = torch.empty(R, dtype=torch.float32, device=rows.device)
    check(lib().mra_lm_head_ce_forward(ptr(rows), max(rows.stride(0), K), R, K, ptr(weight), weight.stride(0), V, dt, ptr(y32), ptr(nll), ptr(lse),
                                       ptr(ws), nbytes, int(want_grad), current_stream()), "mra_lm_head_ce_forward")
    return nll, lse, ws, nbytes


class _LmHeadCE(torch.autograd.Function):
    """ONE node around the two entries.  Nothing of size [R, V] but the workspace's 16-bit P~ is kept; the rows themselves are not saved."""

    @staticmethod
    def forward(ctx, rows, weight, y32, reduction):
        want = ctx.needs_input_grad[0]
        nll, lse, ws, nbytes = _forward_entries(rows, weight, y32, want)
        if want:
            ctx.save_for_backward(weight, y32, lse, ws)
            ctx.cfg = (rows.shape, rows.dtype, nbytes, reduction)
        return nll.mean() if reduction == "mean" else nll

    @staticmethod
    def backward(ctx, grad):
        weight, y32, lse, ws = ctx.saved_tensors
        (R, K), dtype, nbytes, reduction = ctx.cfg
        g = grad.to(torch.float32)
        g = (g / R).expand(R).contiguous() if reduction == "mean" else g.contiguous()      # on the device: no host value is read
        dh = torch.empty(R, K, dtype=dtype, device=weight.device)
        check(lib().mra_lm_head_ce_backward(ptr(g), ptr(weight), weight.stride(0), weight.shape[0], K, mra_dtype(dtype), ptr(y32), ptr(lse), ptr(ws),
                                            nbytes, ptr(dh), K, R, current_stream()), "mra_lm_head_ce_backward")
        return dh, None, None, None


def lm_head_ce_rows(rows: torch.Tensor, weight: torch.Tensor, y: torch.Tensor, *, hip: bool, reduction: str = "mean") -> torch.Tensor:
    """The loss of gathered rows ``rows`` [R, K] with labels ``y`` [R] in [0, V): fp32 ``nll`` [R] (``"none"``) or its mean."""
    if hip and rows.shape[0] > 0:
        if rows.stride(1) != 1 or rows.stride(0) % 8 or rows.stride(0) < rows.shape[1] or rows.data_ptr() % 16:
            rows = rows.contiguous()
        return _LmHeadCE.apply(rows, weight, y.to(torch.int32), reduction)
    ct = torch.float32 if rows.dtype in (torch.float16, torch.bfloat16) else rows.dtype
    z = rows.to(ct) @ weight.to(ct).t()
    if rows.shape[0] == 0:          # no labelled row at all: what torch.nn.functional.cross_entropy gives for an empty batch
        return torch.nn.functional.cross_entropy(z, y, reduction=reduction)
    nll = torch.logsumexp(z, dim=-1) - z.gather(1, y[:, None]).squeeze(1)
    return nll.mean() if reduction == "mean" else nll


def labelled_rows(labels: torch.Tensor):
    """``(index, y)``: the flat positions b * S + t whose NEXT label is not -100, and those labels -- the causal shift of ForCausalLMLoss
    (position t predicts labels[t + 1]; a label at position 0 predicts nothing).  The one host synchronisation: the row count."""
    B, S = labels.shape
    nxt = torch.full_like(labels, IGNORE)
    nxt[:, :-1] = labels[:, 1:]
    flat = nxt.reshape(-1)
    index = torch.nonzero(flat != IGNORE).squeeze(1)
    return index, flat.index_select(0, index)


def lm_head_ce(hidden: torch.Tensor, weight: torch.Tensor, labels: torch.Tensor, *, hip: Optional[bool] = None,
               reduction: str = "mean") -> torch.Tensor:
    """``hidden`` [B, S, K] (the LM's final hidden states, after its last norm), ``weight`` [V, K] (``lm_head.weight``), ``labels`` [B, S]
    unshifted with -100 = ignore.  ``hip=None`` takes the HIP entries when they apply (CUDA, equal 16-bit dtypes, K % 8 == 0, a weight that
    needs no gradient and is stored with 16-byte aligned rows) and the torch route otherwise; ``hip=True`` raises ``MraError`` naming the
    reason; ``hip=False`` is the torch route.  ``reduction`` "mean" (over the labelled rows) or "none" (the per-row nll, in row order)."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
    if hidden.dim() != 3 or labels.shape != hidden.shape[:2] or weight.dim() != 2 or weight.shape[1] != hidden.shape[2]:
        raise ValueError(f"hidden [B, S, K], weight [V, K], labels [B, S] expected, got {tuple(hidden.shape)}, {tuple(weight.shape)}, "
                         f"{tuple(labels.shape)}")
    use = False
    if hip is None or hip:
        why = _hip_reason(hidden, weight)
        if why is not None and hip:
            raise MraError(f"lm_head_ce(hip=True): {why}")
        use = why is None
    index, y = labelled_rows(labels.to(hidden.device))
    rows = hidden.reshape(-1, hidden.shape[-1]).index_select(0, index)       # autograd's scatter carries d rows back into [B, S, K]
    return lm_head_ce_rows(rows, weight, y, hip=use, reduction=reduction)
