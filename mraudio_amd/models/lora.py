"""LoRA adapters on the attached causal LM: the one thing the reference trains (``models/model_utils.py:4-14``: ``r=8``, ``lora_alpha=8``,
``lora_dropout=0.05``, ``bias="none"`` on every linear but ``lm_head``; applied at ``models/xinstructblip.py:147-165``).

Restated from the published algorithm (Hu et al., "LoRA: Low-Rank Adaptation of Large Language Models", 2021) with peft's published
parameter names; ``peft`` itself is absent offline, so parity with it is UNPINNED.  Definition, with a base linear ``y0 = x W^T (+ b)``,
``x`` [M, K], ``W`` [N, K], fp32 master adapters ``A`` [R, K] and ``B`` [N, R], ``s = alpha / R``, keep probability ``q = 1 - p`` and
``op`` = rounding to the LM's dtype (bf16 / f16):

    u[m, j]  = (1/q) sum_k keep(m, k) x[m, k] op(A)[j, k]                    fp32 accumulation, u stays fp32
    y[m, n]  = op(float(y0[m, n]) + s sum_j u[m, j] B[n, j])                 fp32 fma chain, j ascending, written over y0
    du[m, j] = s sum_n g[m, n] op(B)[n, j]                                   g = op(dY)
    dB[n, j] += s sum_m g[m, n] op(u)[m, j]
    dA[j, k] += (1/q) sum_m op(du)[m, j] keep(m, k) x[m, k]
    dx[m, k] = op(float(dx0[m, k]) + (keep(m, k) / q) sum_j du[m, j] A[j, k])     dx0 = g W from torch, updated in place

Every operand of a matrix-core product is rounded to the operand dtype and accumulated in fp32; every rank-R update is an fp32 chain.
Dropout is counter based: ``keep(seed, m, k)`` is a pure integer function (``keep_mask`` here, ``lora_keep`` in ``csrc/lora.hip``, the same
bits), so the backward regenerates the mask and none is stored.  ``p = 0`` or eval mode hashes nothing.

On the GPU with a 16-bit LM the low-rank part runs on the HIP entries ``mra_lora_down`` / ``mra_lora_up_add`` / ``mra_lora_wgrad`` (2 launches
forward, 4 backward, in place on the base products, which stay stock torch matmuls); on the CPU, or with ``hip=False``, the same arithmetic
runs as torch ops under torch.autograd -- the oracle of the tests.  Out of scope: 8-bit base weights (bitsandbytes), merging the adapters
into ``W``, LoRA on the Q-Formers."""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional

import torch
from torch import nn

from .._lib import MRA_LORA_NR, MRA_LORA_RN, MraError, check, current_stream, lib, mra_dtype, ptr

_M32 = 0xFFFFFFFF
KEY_PREFIX = "base_model.model."       # peft's PeftModel -> LoraModel -> the wrapped LM
ADAPTER = "default"


# ---- counter-based dropout ------------------------------------------------------------------------------------------------------------
def keep_threshold(p: float) -> int:
    """``floor(p 2^32 + 0.5)`` clamped to 32 bits: a hash below it drops the element (the C entries compute the same value)."""
    return min(int(math.floor(float(p) * 4294967296.0 + 0.5)), _M32)


def keep_hash(idx: torch.Tensor, seed: int) -> torch.Tensor:
    """The two-multiply "lowbias32" finaliser over ``lo32(idx) ^ seed_lo ^ hi32(idx) * 0x9E3779B9 ^ seed_hi``: int64 in, values in
    [0, 2^32) out (int64 products wrap modulo 2^64, which leaves the low 32 bits right)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    h = (idx & _M32) ^ (seed & _M32) ^ (((idx >> 32) * 0x9E3779B9) & _M32) ^ (seed >> 32)
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & _M32
    h = h ^ (h >> 15)
    h = (h * 0x846CA68B) & _M32
    return h ^ (h >> 16)


def keep_mask(seed: int, rows: int, width: int, p: float, device=None) -> torch.Tensor:
    """bool [rows, width]: element (m, k) has index ``m * width + k``.  ``p = 0`` keeps all, without hashing."""
    if p <= 0.0:
        return torch.ones(rows, width, dtype=torch.bool, device=device)
    idx = torch.arange(rows, dtype=torch.int64, device=device)[:, None] * width + torch.arange(width, dtype=torch.int64, device=device)[None, :]
    return keep_hash(idx, seed) >= keep_threshold(p)


# ---- the HIP entries --------------------------------------------------------------------------------------------------------------------
def _rows16(t: torch.Tensor) -> torch.Tensor:
    """A [M, width] tensor the entries take: unit column stride, a pitch of whole 16-byte groups, a 16-byte aligned base."""
    if t.stride(1) != 1 or t.stride(0) % 8 or t.stride(0) < t.shape[1] or t.data_ptr() % 16:
        t = t.contiguous()
        if t.data_ptr() % 16:
            t = t.clone(memory_format=torch.contiguous_format)
    return t


def lora_down(x: torch.Tensor, w: torch.Tensor, layout: int, scale: float, p: float = 0.0, seed: int = 0, out: Optional[torch.Tensor] = None):
    """``out [M, R] fp32 = scale * drop(x) op(w)^T`` (``mra_lora_down``); ``w`` fp32, [R, K] (``MRA_LORA_RN``) or [K, R] (``MRA_LORA_NR``)."""
    M, K = x.shape
    R = w.shape[0] if layout == MRA_LORA_RN else w.shape[1]
    if out is None:
        out = torch.empty(M, R, dtype=torch.float32, device=x.device)
    check(lib().mra_lora_down(ptr(x), x.stride(0) if M > 1 else max(x.stride(0), K), M, K, mra_dtype(x.dtype), ptr(w), R, layout, float(scale), float(p),
                              int(seed), ptr(out), current_stream()), "mra_lora_down")
    return out


def lora_up_add(y: torch.Tensor, u: torch.Tensor, w: torch.Tensor, layout: int, scale: float, p: float = 0.0, seed: int = 0) -> torch.Tensor:
    """``y = op(float(y) + scale * keep * u w)`` in place (``mra_lora_up_add``); ``w`` fp32, [N, R] (``MRA_LORA_NR``) or [R, N]."""
    M, N = y.shape
    check(lib().mra_lora_up_add(ptr(y), y.stride(0) if M > 1 else max(y.stride(0), N), M, N, mra_dtype(y.dtype), ptr(u), u.shape[1], ptr(w), layout,
                                float(scale), float(p), int(seed), current_stream()), "mra_lora_up_add")
    return y


def lora_wgrad(x: torch.Tensor, u: torch.Tensor, dw: torch.Tensor, layout: int, scale: float, p: float = 0.0, seed: int = 0) -> torch.Tensor:
    """``dw += scale * drop(x)^T op(u)`` (``mra_lora_wgrad``); ``dw`` fp32, [N, R] (``MRA_LORA_NR``) or [R, N]."""
    M, N = x.shape
    check(lib().mra_lora_wgrad(ptr(x), x.stride(0) if M > 1 else max(x.stride(0), N), M, N, mra_dtype(x.dtype), ptr(u), u.shape[1], ptr(dw), layout,
                               float(scale), float(p), int(seed), current_stream()), "mra_lora_wgrad")
    return dw


class _LoraHip(torch.autograd.Function):
    """ONE node per adapted linear: the base products ``x W^T`` and ``dY W`` are torch matmuls inside it, the low-rank part the HIP entries in
    place on their results.  ``unscale`` (1 / loss_scale) is folded into the scales of the two weight gradients, in fp32."""

    @staticmethod
    def forward(ctx, x, W, b, A, B, s, p, seed, unscale):
        K, N = W.shape[1], W.shape[0]
        x2 = _rows16(x.reshape(-1, K))
        y = nn.functional.linear(x2, W, b)
        inv_q = 1.0 / (1.0 - p)
        u = lora_down(x2, A, MRA_LORA_RN, inv_q, p, seed)
        lora_up_add(y, u, B, MRA_LORA_NR, s)
        ctx.save_for_backward(x2, u, W, A, B)
        ctx.cfg = (s, p, seed, unscale, inv_q)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, u, W, A, B = ctx.saved_tensors
        s, p, seed, unscale, inv_q = ctx.cfg
        g = _rows16(dy.reshape(-1, W.shape[0]).to(x2.dtype))
        du = lora_down(g, B, MRA_LORA_NR, s)
        dB = lora_wgrad(g, u, torch.zeros_like(B), MRA_LORA_NR, s * unscale) if ctx.needs_input_grad[4] else None
        dA = lora_wgrad(x2, du, torch.zeros_like(A), MRA_LORA_RN, inv_q * unscale, p, seed) if ctx.needs_input_grad[3] else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.matmul(g, W)
            lora_up_add(dx, du, A, MRA_LORA_RN, inv_q, p, seed)
            dx = dx.view(*dy.shape[:-1], W.shape[1])
        return dx, None, None, dA, dB, None, None, None, None


class _GradScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, k):
        ctx.k = k
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.k, None


def lora_torch(x, W, b, A, B, s: float, p: float, seed: int, unscale: float = 1.0):
    """The definition as torch ops under torch.autograd (any float dtype; 16-bit inputs compute in fp32): the CPU path and the oracle."""
    K, N = W.shape[1], W.shape[0]
    ct = torch.float32 if x.dtype in (torch.float16, torch.bfloat16) else x.dtype
    if unscale != 1.0:
        A, B = _GradScale.apply(A, unscale), _GradScale.apply(B, unscale)
    x2 = x.reshape(-1, K)
    y0 = nn.functional.linear(x2, W, b)
    if p > 0.0:
        x2 = x2 * keep_mask(seed, x2.shape[0], K, p, x.device).to(x.dtype)
    u = (x2.to(ct) @ A.to(x.dtype).to(ct).t()) * (1.0 / (1.0 - p))
    y = (y0.to(ct) + s * (u @ B.to(ct).t())).to(x.dtype)
    return y.view(*x.shape[:-1], N)


# ---- the module ---------------------------------------------------------------------------------------------------------------------------
class LoraLinear(nn.Module):
    """One frozen ``nn.Linear`` with a rank-``r`` adapter.  Parameters are addressed as peft addresses them: ``<path>.base_layer.weight``,
    ``<path>.lora_A.default.weight`` [r, in], ``<path>.lora_B.default.weight`` [out, r].  The adapters are fp32 masters on the base weight's
    device (a later ``.to(dtype)`` of the LM would round them: apply the adapters after the cast).  A is kaiming-uniform with ``a = sqrt(5)``,
    B zero, so a fresh adapter leaves the output unchanged, bit for bit.  ``hip``: None = the HIP entries on a GPU with a 16-bit input they take (the base weight's dtype,
    r <= 16, widths that are multiples of 8), torch ops otherwise; False = torch ops; True = the HIP entries or an error.  ``grad_unscale``: adapter gradients are multiplied by it in fp32
    (``XInstructBLIP.loss_scale`` sets 1 / loss_scale).  One seed per forward call from torch's default CPU generator: ``torch.manual_seed``
    and activation checkpointing (which restores the CPU generator) reproduce the mask."""

    def __init__(self, base: nn.Linear, r: int = 8, alpha: float = 8, dropout: float = 0.05, hip: Optional[bool] = None):
        super().__init__()
        if not isinstance(base, nn.Linear):
            raise TypeError("LoraLinear wraps an nn.Linear")
        if r < 1:
            raise ValueError("r must be >= 1")
        if not 0.0 <= dropout < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        self.base_layer = base.requires_grad_(False)
        self.in_features, self.out_features = base.in_features, base.out_features
        self.r, self.lora_alpha, self.dropout, self.scaling = int(r), float(alpha), float(dropout), float(alpha) / int(r)
        self.hip, self.grad_unscale, self.last_seed = hip, 1.0, 0
        dev = base.weight.device
        dt = torch.float64 if base.weight.dtype == torch.float64 else torch.float32
        self.lora_A = nn.ModuleDict({ADAPTER: nn.Linear(self.in_features, self.r, bias=False, device=dev, dtype=dt)})
        self.lora_B = nn.ModuleDict({ADAPTER: nn.Linear(self.r, self.out_features, bias=False, device=dev, dtype=dt)})
        nn.init.kaiming_uniform_(self.lora_A[ADAPTER].weight, a=math.sqrt(5))
        nn.init.zeros_(self.lora_B[ADAPTER].weight)

    def _use_hip(self, x: torch.Tensor) -> bool:
        if self.hip is False:
            return False
        fits_input = x.is_cuda and x.dtype in (torch.float16, torch.bfloat16) and x.dtype == self.base_layer.weight.dtype
        fits_shape = self.r <= 16 and self.in_features % 8 == 0 and self.out_features % 8 == 0
        if self.hip is None:        # the automatic choice never raises: what the entries do not take runs as torch ops
            return fits_input and fits_shape
        if not fits_input:
            raise MraError("the HIP LoRA path needs a GPU input in the base weight's 16-bit dtype")
        if not fits_shape:
            raise MraError(f"the HIP LoRA path needs r <= 16 and widths that are multiples of 8 (r {self.r}, {self.in_features} -> {self.out_features})")
        return True

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        A, B = self.lora_A[ADAPTER].weight, self.lora_B[ADAPTER].weight
        p = self.dropout if self.training else 0.0
        seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item()) if p > 0.0 else 0
        self.last_seed = seed
        W, b = self.base_layer.weight, self.base_layer.bias
        if self._use_hip(x):
            return _LoraHip.apply(x, W, b, A, B, self.scaling, p, seed, float(self.grad_unscale))
        return lora_torch(x, W, b, A, B, self.scaling, p, seed, float(self.grad_unscale))

    def extra_repr(self) -> str:
        return f"r={self.r}, alpha={self.lora_alpha}, dropout={self.dropout}"


def lora_modules(llm: nn.Module) -> Dict[str, LoraLinear]:
    return {n: m for n, m in llm.named_modules() if isinstance(m, LoraLinear)}


def apply_lora(llm: nn.Module, r: int = 8, alpha: float = 8, dropout: float = 0.05, target_modules: Optional[Iterable[str]] = None,
               hip: Optional[bool] = None) -> List[str]:
    """Wrap every ``nn.Linear`` of ``llm`` except ``lm_head`` (the reference's ``find_all_linear_names`` with its 16-bit class,
    ``models/model_utils.py:17-27``; ``target_modules``: leaf names to keep instead) and freeze everything else, as peft does.  Returns the
    wrapped module paths.  A module that is already adapted is left alone."""
    inside = tuple(f"{n}." for n in lora_modules(llm))
    want = None if target_modules is None else set(target_modules)
    found = []
    for name, mod in llm.named_modules():
        leaf = name.split(".")[-1]
        if not isinstance(mod, nn.Linear) or not name or name.startswith(inside):
            continue
        if leaf == "lm_head" if want is None else leaf not in want:
            continue
        found.append((name, mod))
    llm.requires_grad_(False)
    for name, mod in found:
        parent = llm.get_submodule(name.rpartition(".")[0]) if "." in name else llm
        setattr(parent, name.split(".")[-1], LoraLinear(mod, r, alpha, dropout, hip))
    for m in lora_modules(llm).values():
        m.lora_A.requires_grad_(True)
        m.lora_B.requires_grad_(True)
    return [n for n, _ in found]


def lora_parameters(llm: nn.Module) -> List[nn.Parameter]:
    """The adapter parameters in module order: A then B of every adapted linear."""
    return [p for m in lora_modules(llm).values() for p in (m.lora_A[ADAPTER].weight, m.lora_B[ADAPTER].weight)]


def lora_state_dict(llm: nn.Module) -> Dict[str, torch.Tensor]:
    """``base_model.model.<module path>.lora_{A,B}.default.weight`` -> tensor: the keys a peft-wrapped LM gives its adapters."""
    out = {}
    for n, m in lora_modules(llm).items():
        out[f"{KEY_PREFIX}{n}.lora_A.{ADAPTER}.weight"] = m.lora_A[ADAPTER].weight.detach()
        out[f"{KEY_PREFIX}{n}.lora_B.{ADAPTER}.weight"] = m.lora_B[ADAPTER].weight.detach()
    return out


def load_lora_state_dict(llm: nn.Module, sd: Dict[str, torch.Tensor]):
    """Copy adapter tensors in; returns ``(missing, unexpected)`` key lists (nothing raises: the caller decides)."""
    own = lora_state_dict(llm)
    with torch.no_grad():
        for k, v in sd.items():
            if k in own:
                if own[k].shape != v.shape:
                    raise RuntimeError(f"{k}: shape {tuple(v.shape)} in the file, {tuple(own[k].shape)} in the model")
                own[k].copy_(v)
    return [k for k in own if k not in sd], [k for k in sd if k not in own]
