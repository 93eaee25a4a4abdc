"""The attached LM's greedy decode, one whole token per C call (``mra_lm_step``, ``csrc/lm_step.hip``).

The reference decodes with ``self.llm_model.generate(inputs_embeds=..., attention_mask=..., max_new_tokens=64)``
(``models/xinstructblip.py:383-391``, ``utils/trainer.py:157-165``).  Behind the prefill every new token is a forward over ONE row per sequence:
pure weight streaming, issued by ``generate`` as a few dozen small launches per layer from Python.  Here:

    lm_step_ref(llm, h_or_tokens, cache, mask, positions, slot)   the definition of one step as torch ops (float64 / fp32 on the CPU, any dtype on
                                                                  either device) with the kernels' roundings -- the oracle of the tests
    HipLmDecoder(llm)                                             walks a Llama-shaped ``*ForCausalLM`` and builds the descriptor from the
                                                                  parameters as they lie (no weight is copied: tied embeddings work)
    HipLmDecoder.generate(inputs_embeds, attention_mask, n)       prefill through the LM's own forward, its K/V copied once into a static
                                                                  buffer, then one ``mra_lm_step`` per token with no torch op in between
    HipLmDecoder(llm, prefill="hip")                              that forward runs inside ``hip_decode(llm, prefill=True)``: its attention is
                                                                  ``mra_prefill_attention`` under the key mask, with no [S, S] mask tensor

Where the kernels round (``dtype``), one rounding each: the residual stream, q / k / v, the attention output, the SwiGLU activation.  Everything
inside a launch is fp32: the RMSNorm rows ``(x * rsqrt(mean(x^2) + eps)) * gain`` are an fp32 copy, the LoRA term ``scale * (x A^T) B^T`` is added
to the fp32 product BEFORE the rotation, the logits are fp32.  (transformers rounds the normalised rows to the LM's dtype twice; this route does
not, which is the finer of the two.)

Out of scope: graph capture, a persistent whole-layer kernel, the prefill's linears, norms and rotary, sampling and beam search, logits processors, paged or quantised
K/V, 8-bit base weights, merged adapters, architectures that are not Llama-shaped, more than 8 sequences inside one launch."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from .. import _lib
from .._lib import MraError, check, current_stream, lib, mra_dtype
from .lm_decode import GROUPS, HEAD_DIMS, _torch_ops, hip_decode
from .lora import ADAPTER, LoraLinear

MAX_B, MAX_R, MAX_EOS = 8, 16, 8
PREFILLS = ("stock", "hip")
LINEARS = ("q", "k", "v", "o", "gate", "up", "down")
# the named wrong versions of the step the tests must tell from the right one (tests/lm_step_cases.py)
MUTANTS = ("rotate_half_sign", "position_from_slot", "slot_from_position", "lora_scale_dropped", "lora_after_rotation", "residual_dropped",
           "gain_before_rsqrt", "head_modulo_groups", "silu_on_up")


# ---- the definition, piece by piece -------------------------------------------------------------------------------------------------------------
def _rd(x: torch.Tensor, dtype: Optional[torch.dtype]) -> torch.Tensor:
    """One rounding to ``dtype`` and back (None: none)."""
    return x if dtype is None else x.to(dtype).to(x.dtype)


def split_linear(mod) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor], float]:
    """``(W, A, B, scale)`` of an ``nn.Linear`` or a ``LoraLinear`` around one (A, B None without an adapter)."""
    if isinstance(mod, LoraLinear):
        return mod.base_layer.weight, mod.lora_A[ADAPTER].weight, mod.lora_B[ADAPTER].weight, float(mod.scaling)
    return mod.weight, None, None, 0.0


def linear_ref(x: torch.Tensor, W: torch.Tensor, A=None, Bw=None, scale: float = 0.0, mutant: Optional[str] = None) -> torch.Tensor:
    """``x W^T + scale (x A^T) B^T`` in x's type."""
    y = x @ W.to(x.dtype).T
    if A is not None:
        t = (x @ A.to(x.dtype).T) @ Bw.to(x.dtype).T
        y = y + (t if mutant == "lora_scale_dropped" else scale * t)
    return y


def rms_ref(x: torch.Tensor, gain: torch.Tensor, eps: float, mutant: Optional[str] = None) -> torch.Tensor:
    """``(x * rsqrt(mean(x^2) + eps)) * gain`` in x's type.  The mutant ``gain_before_rsqrt`` is a reading of "gain applied before the rsqrt
    factor": here nothing between x and the gain is rounded to 16 bits (the rows stay fp32), so the placement of the gain relative to a
    ROUNDING has no counterpart in this definition (in fp32 the two orders differ by an ulp, which no bound can tell apart); the mutant
    moves the gain in front of the statistics instead -- the error a misplaced gain can still make in this route."""
    g = gain.to(x.dtype)
    if mutant == "gain_before_rsqrt":                      # the gain inside the statistics: the rsqrt factor of the gained rows
        x = x * g
        return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return (x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)) * g


def rope_ref(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, mutant: Optional[str] = None) -> torch.Tensor:
    """``x`` [B, H, D], ``cos`` / ``sin`` [B, D]: transformers' Llama ``x cos + rotate_half(x) sin`` over the pairs (i, i + D/2)."""
    h = x.shape[-1] // 2
    rot = torch.cat([-x[..., h:], x[..., :h]], -1)
    if mutant == "rotate_half_sign":
        rot = -rot
    return x * cos[:, None, :].to(x.dtype) + rot * sin[:, None, :].to(x.dtype)


def swiglu_ref(g: torch.Tensor, u: torch.Tensor, mutant: Optional[str] = None) -> torch.Tensor:
    if mutant == "silu_on_up":
        g, u = u, g
    return g * torch.sigmoid(g) * u


def attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: torch.Tensor, scale: float, mutant: Optional[str] = None) -> torch.Tensor:
    """``q`` [B, Hq, D], ``k`` / ``v`` [B, Hkv, S, D], ``mask`` [B, S] (nonzero = attend): [B, Hq, D] in q's type; query head h reads kv head h / G.
    The one-token case of ``lm_decode``'s definition (the row sits at the last slot); a masked slot's bits reach nothing."""
    if mutant == "head_modulo_groups":                     # the wrong kv head per query head, handed over as Hq kv heads of one query head each
        idx = torch.arange(q.shape[1], device=q.device) % k.shape[1]
        k, v = k[:, idx], v[:, idx]
    return _torch_ops(q[:, :, None], k, v, mask.to(torch.bool)[:, None, None], scale, k.shape[2] - 1)[0][:, :, 0]


def argmax_ref(logits: torch.Tensor, mutant: Optional[str] = None) -> torch.Tensor:
    """The first maximum of each row; a NaN counts as the maximum and the first NaN wins (``torch.argmax``'s order, stated and tested)."""
    z = torch.where(torch.isnan(logits), torch.full_like(logits, float("inf")), logits)
    nan = torch.isnan(logits)
    V = logits.shape[-1]
    idx = torch.arange(V, device=logits.device).expand_as(logits)
    if nan.any():
        z = torch.where(nan.any(-1, keepdim=True), nan.to(logits.dtype), z)                    # among NaNs only the NaNs compete
    best = z.max(-1, keepdim=True).values
    hit = z == best
    if mutant == "argmax_tie_highest":
        return torch.where(hit, idx, torch.full_like(idx, -1)).max(-1).values
    return torch.where(hit, idx, torch.full_like(idx, V)).min(-1).values


def greedy_ref(argmax: torch.Tensor, finished: torch.Tensor, pad: int, eos: List[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """generate's bookkeeping for one step: a finished sequence emits ``pad``; a sequence that emits an eos id becomes finished."""
    tok = torch.where(finished.to(torch.bool), torch.full_like(argmax, pad), argmax)
    stop = torch.zeros_like(tok, dtype=torch.bool)
    for e in eos:
        stop |= tok == e
    return tok, finished.to(torch.bool) | stop


# ---- the LM, walked -----------------------------------------------------------------------------------------------------------------------------
def _refuse(what: str):
    raise MraError(f"HipLmDecoder: {what}")


def walk(llm) -> Dict:
    """The pieces of a Llama-shaped ``*ForCausalLM`` (modules, not copies); ``MraError`` naming what was found for anything else."""
    model = getattr(llm, "model", None)
    layers = getattr(model, "layers", None)
    if model is None or layers is None or not hasattr(llm, "lm_head") or not hasattr(model, "embed_tokens") or not hasattr(model, "norm") \
            or not hasattr(model, "rotary_emb"):
        _refuse(f"a Llama-shaped *ForCausalLM (model.embed_tokens, model.layers, model.norm, model.rotary_emb, lm_head) is expected, found "
                f"{type(llm).__name__}")
    cfg = llm.config
    act = getattr(cfg, "hidden_act", None)
    if act != "silu":
        _refuse(f"hidden_act must be 'silu', found {act!r}")
    if getattr(cfg, "sliding_window", None) is not None and any(t != "full_attention" for t in (getattr(cfg, "layer_types", None) or ["sliding"])):
        _refuse(f"sliding-window attention is not taken (sliding_window = {cfg.sliding_window})")
    for name in ("attn_logit_softcapping", "final_logit_softcapping"):
        if getattr(cfg, name, None) is not None:
            _refuse(f"soft caps are not taken ({name} = {getattr(cfg, name)})")

    def norm(mod, where):
        eps = getattr(mod, "variance_epsilon", getattr(mod, "eps", None))
        if "RMSNorm" not in type(mod).__name__ or getattr(mod, "weight", None) is None or eps is None or getattr(mod, "bias", None) is not None:
            _refuse(f"{where} must be an RMSNorm with a gain and no bias, found {type(mod).__name__}")
        return mod.weight, float(eps)

    def linear(mod, where):
        base = mod.base_layer if isinstance(mod, LoraLinear) else mod
        if not isinstance(base, nn.Linear):
            _refuse(f"{where} must be an nn.Linear or a LoraLinear around one, found {type(mod).__name__}")
        if base.bias is not None:
            _refuse(f"{where} has a bias; biased linears are not taken")
        return mod

    out = {"layers": [], "embed": model.embed_tokens.weight, "rotary": model.rotary_emb}
    out["final_norm"], out["eps"] = norm(model.norm, "model.norm")
    if not isinstance(llm.lm_head, nn.Linear) or llm.lm_head.bias is not None:
        _refuse(f"lm_head must be an nn.Linear without a bias, found {type(llm.lm_head).__name__}")
    out["head"] = llm.lm_head.weight
    for i, layer in enumerate(layers):
        at, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
        if at is None or mlp is None:
            _refuse(f"layer {i} has no self_attn / mlp, found {type(layer).__name__}")
        for extra in ("q_norm", "k_norm"):
            if hasattr(at, extra):
                _refuse(f"layer {i} self_attn has {extra}; only Llama-shaped attention is taken")
        rec = {}
        for short, owner, name in (("q", at, "q_proj"), ("k", at, "k_proj"), ("v", at, "v_proj"), ("o", at, "o_proj"), ("gate", mlp, "gate_proj"),
                                   ("up", mlp, "up_proj"), ("down", mlp, "down_proj")):
            if not hasattr(owner, name):
                _refuse(f"layer {i} has no {name} (found {type(owner).__name__}: {', '.join(n for n, _ in owner.named_children())})")
            rec[short] = linear(getattr(owner, name), f"layer {i} {name}")
        rec["norm1"], e1 = norm(layer.input_layernorm, f"layer {i} input_layernorm")
        rec["norm2"], e2 = norm(layer.post_attention_layernorm, f"layer {i} post_attention_layernorm")
        if e1 != out["eps"] or e2 != out["eps"]:
            _refuse(f"one eps for every RMSNorm is expected, found {e1}, {e2} and {out['eps']}")
        rec["scale"] = float(getattr(at, "scaling", at.head_dim ** -0.5))
        rec["D"] = int(at.head_dim)
        out["layers"].append(rec)
    D = out["layers"][0]["D"]
    out.update(D=D, Hq=cfg.num_attention_heads, Hkv=cfg.num_key_value_heads, hidden=cfg.hidden_size, inter=cfg.intermediate_size,
               V=out["head"].shape[0], scale=out["layers"][0]["scale"])
    return out


def rope_table(llm, n: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 ``cos`` / ``sin`` [n, D] for the positions 0 .. n - 1 from the LM's own rotary module (its rope type, not a restatement)."""
    rot = llm.model.rotary_emb
    cos, sin = rot(torch.zeros(1, dtype=torch.float32, device=device), torch.arange(n, device=device)[None])
    return cos[0].float().contiguous(), sin[0].float().contiguous()


@torch.no_grad()
def lm_step_ref(llm, h_or_tokens: torch.Tensor, cache: torch.Tensor, mask: torch.Tensor, positions: torch.Tensor, slot: int,
                dtype: Optional[torch.dtype] = None, compute: torch.dtype = torch.float32, mutant: Optional[str] = None,
                rope: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One token through ``llm`` as ``mra_lm_step`` defines it.  ``h_or_tokens``: [B, hidden] rows, or integer token ids [B]; ``cache``
    [L, 2, B, Hkv, Smax, D] (slot ``slot`` of every layer is WRITTEN, in the cache's own dtype); ``mask`` [B, Smax] with nonzero = attend (the
    caller has set column ``slot``); ``positions`` [B] rotary positions of the token.  ``dtype``: the type the kernels round to at the places the
    module docstring lists (None: no rounding -- the plain forward in ``compute``).  Returns ``(logits [B, V], final hidden rows [B, hidden])``
    in ``compute``.  ``rope``: a ``rope_table`` to index instead of asking the module."""
    w = walk(llm)
    ct, dev = compute, cache.device
    if h_or_tokens.dtype in (torch.int32, torch.int64):
        h = w["embed"][h_or_tokens.long()].to(ct)
    else:
        h = h_or_tokens.to(ct)
    h = _rd(h, dtype)
    S = slot + 1
    pos = positions.long()
    if mutant == "position_from_slot":
        pos = torch.full_like(pos, slot)
    cos, sin = rope if rope is not None else rope_table(llm, int(pos.max()) + 1, dev)
    cos, sin = cos[pos].to(ct), sin[pos].to(ct)
    B, Hq, Hkv, D = h.shape[0], w["Hq"], w["Hkv"], w["D"]
    for l, rec in enumerate(w["layers"]):
        xn = rms_ref(h, rec["norm1"], w["eps"], mutant)
        q, k, v = (linear_ref(xn, *split_linear(rec[n]), mutant=None if mutant == "lora_after_rotation" else mutant) for n in ("q", "k", "v"))
        if mutant == "lora_after_rotation":               # the base product is rotated, the adapter term is added unrotated
            base = [xn @ split_linear(rec[n])[0].to(ct).T for n in ("q", "k")]
            q = rope_ref(base[0].view(B, Hq, D), cos, sin) + (q - base[0]).view(B, Hq, D)
            k = rope_ref(base[1].view(B, Hkv, D), cos, sin) + (k - base[1]).view(B, Hkv, D)
        else:
            q, k = rope_ref(q.view(B, Hq, D), cos, sin, mutant), rope_ref(k.view(B, Hkv, D), cos, sin, mutant)
        q, k, v = _rd(q, dtype), _rd(k, dtype), _rd(v.view(B, Hkv, D), dtype)
        if mutant == "slot_from_position":
            for b in range(B):
                cache[l, 0, b, :, int(pos[b])], cache[l, 1, b, :, int(pos[b])] = k[b].to(cache.dtype), v[b].to(cache.dtype)
        else:
            cache[l, 0, :, :, slot], cache[l, 1, :, :, slot] = k.to(cache.dtype), v.to(cache.dtype)
        ao = _rd(attention_ref(q, cache[l, 0, :, :, :S], cache[l, 1, :, :, :S], mask[:, :S], rec["scale"], mutant), dtype).reshape(B, Hq * D)
        o = linear_ref(ao, *split_linear(rec["o"]), mutant=mutant)
        h = _rd(o if mutant == "residual_dropped" else h + o, dtype)
        xn = rms_ref(h, rec["norm2"], w["eps"], mutant)
        act = _rd(swiglu_ref(linear_ref(xn, *split_linear(rec["gate"]), mutant=mutant), linear_ref(xn, *split_linear(rec["up"]), mutant=mutant), mutant), dtype)
        dn = linear_ref(act, *split_linear(rec["down"]), mutant=mutant)
        h = _rd(dn if mutant == "residual_dropped" else h + dn, dtype)
    logits = rms_ref(h, w["final_norm"], w["eps"], mutant) @ w["head"].to(ct).T
    return logits, h


# ---- the decoder --------------------------------------------------------------------------------------------------------------------------------
def step_workspace_bytes(B: int, hidden: int, inter: int, Hq: int, D: int, Smax: int) -> int:
    """include/mra.h's formula, restated (the tests hold the two together)."""
    up = lambda n: (n + 255) // 256 * 256
    rows = B * Hq * ((Smax + 255) // 256)
    return up(4 * B * hidden) + 3 * up(4 * B * MAX_R) + 2 * up(2 * B * Hq * D) + up(2 * B * inter) + 2 * up(4 * rows) + up(4 * rows * D)


class HipLmDecoder:
    """Greedy decode of a Llama-shaped ``*ForCausalLM`` with one ``mra_lm_step`` per token.  The descriptor points at the parameters as they
    lie; it is rebuilt when a parameter's ``data_ptr`` or an adapter (rank, scale) changes.  The LM itself is never modified."""

    check_every = 8                 # steps between two looks of the host at ``finished`` (each look is a synchronisation)

    def __init__(self, llm, ref: bool = False, prefill: str = "stock"):
        """``ref``: every step runs ``lm_step_ref`` + ``argmax_ref`` + ``greedy_ref`` instead of ``mra_lm_step`` (any device and dtype): the
        same loop around the definition, which is how the tests hold the loop against ``generate`` without a GPU.  ``prefill``: "stock" (the
        LM's forward as it is configured) or "hip" (the same forward inside ``lm_decode.hip_decode(llm, prefill=True)``; the LM's attention
        implementation is put back afterwards, also after an exception)."""
        if prefill not in PREFILLS:
            raise ValueError(f"prefill must be one of {PREFILLS}, got {prefill!r}")
        self.llm = llm
        self.ref = ref
        self.prefill = prefill
        self._sig = None
        self._walk = None
        self._layers = None
        walk(llm) if ref else self.validate()

    @staticmethod
    def _vector(t: torch.Tensor, dt: torch.dtype, where: str, rows: bool = False):
        """A gain vector (or, ``rows``, the embedding table) as the kernels read it: the LM's 16-bit dtype, unit stride, 16-byte rows."""
        if t.dtype != dt or t.stride(-1) != 1 or (rows and (t.dim() != 2 or t.stride(0) % 8)):
            _refuse(f"{where} must be {dt} with unit stride{' and a pitch that is a multiple of 8' if rows else ''}, found {t.dtype} {tuple(t.stride())}")

    def validate(self) -> Dict:
        w = walk(self.llm)
        dt = w["head"].dtype
        if dt not in (torch.float16, torch.bfloat16):
            _refuse(f"the LM must be in float16 or bfloat16, found {dt}")
        if w["D"] not in HEAD_DIMS or w["Hq"] % w["Hkv"] or w["Hq"] // w["Hkv"] not in GROUPS:
            _refuse(f"head_dim {w['D']} with {w['Hq']} / {w['Hkv']} heads is outside D in {HEAD_DIMS}, Hq / Hkv in {GROUPS}")
        self._vector(w["final_norm"], dt, "model.norm.weight")
        self._vector(w["embed"], dt, "embed_tokens.weight", rows=True)
        if w["head"].stride(1) != 1 or w["head"].stride(0) % 8:
            _refuse(f"lm_head.weight must have unit stride along K and a pitch that is a multiple of 8, found {tuple(w['head'].stride())}")
        if w["hidden"] % 8 or w["inter"] % 8:
            _refuse(f"hidden {w['hidden']} and intermediate {w['inter']} must be multiples of 8")
        for i, rec in enumerate(w["layers"]):
            for n in ("norm1", "norm2"):
                self._vector(rec[n], dt, f"layer {i} {n}")
            for n in LINEARS:
                W, A, Bw, _ = split_linear(rec[n])
                if W.dtype != dt or W.stride(1) != 1 or W.stride(0) % 8:
                    _refuse(f"layer {i} {n}: the weight must be {dt}, unit stride along K and a pitch that is a multiple of 8, found {W.dtype} {W.stride()}")
                if A is not None and (A.dtype != torch.float32 or Bw.dtype != torch.float32 or A.shape[0] > MAX_R or not A.is_contiguous() or not Bw.is_contiguous()):
                    _refuse(f"layer {i} {n}: adapters must be contiguous fp32 masters of rank <= {MAX_R}, found {A.dtype} rank {A.shape[0]}")
        return w

    # the pointer table -------------------------------------------------------------------------------------------------------------------------
    def _signature(self, w) -> tuple:
        sig = [w["embed"].data_ptr(), w["head"].data_ptr(), w["final_norm"].data_ptr()]
        for rec in w["layers"]:
            sig += [rec["norm1"].data_ptr(), rec["norm2"].data_ptr()]
            for n in LINEARS:
                W, A, Bw, s = split_linear(rec[n])
                sig += [W.data_ptr(), W.stride(0), 0 if A is None else A.data_ptr(), 0 if A is None else Bw.data_ptr(), 0 if A is None else A.shape[0], s]
        return tuple(sig)

    def _table(self):
        w = self.validate()
        sig = self._signature(w)
        if sig != self._sig:
            arr = (_lib.mra_lm_layer * len(w["layers"]))()
            for rec, y in zip(w["layers"], arr):
                y.norm1, y.norm2 = rec["norm1"].data_ptr(), rec["norm2"].data_ptr()
                for n in LINEARS:
                    W, A, Bw, s = split_linear(rec[n])
                    lin = getattr(y, n)
                    lin.W, lin.ldw, lin.N = W.data_ptr(), W.stride(0), W.shape[0]
                    if A is not None:
                        lin.A, lin.Bw, lin.R, lin.scale = A.data_ptr(), Bw.data_ptr(), A.shape[0], s
            self._sig, self._layers = sig, arr
        self._walk = w
        return w, self._layers

    def descriptor(self, B: int, cache: torch.Tensor, mask8: torch.Tensor, position: torch.Tensor, rope, h: torch.Tensor, logits: torch.Tensor,
                   finished: Optional[torch.Tensor], ws: torch.Tensor, pad: int, eos: List[int]) -> _lib.mra_lm_step_desc:
        """The descriptor of a step over ``cache`` [L, 2, B, Hkv, Smax, D]; ``slot``, ``pos_offset``, ``tokens_in`` and ``tokens_out`` are set per step."""
        w, layers = self._table()
        L, _, Bc, Hkv, Smax, D = cache.shape
        if Bc != B or L != len(w["layers"]) or Hkv != w["Hkv"] or D != w["D"] or cache.dtype != w["head"].dtype:
            _refuse(f"the cache {tuple(cache.shape)} {cache.dtype} is not this LM's")
        for l, y in enumerate(layers):
            y.kcache, y.vcache = cache[l, 0].data_ptr(), cache[l, 1].data_ptr()
        d = _lib.mra_lm_step_desc()
        d.struct_bytes = C.sizeof(_lib.mra_lm_step_desc)
        d.B, d.hidden, d.intermediate, d.Hq, d.Hkv, d.D, d.L, d.V = B, w["hidden"], w["inter"], w["Hq"], Hkv, D, L, w["V"]
        d.dtype, d.Smax, d.eps, d.attn_scale = mra_dtype(cache.dtype), Smax, w["eps"], w["scale"]
        d.layers = layers
        d.embed, d.ld_embed, d.final_norm = w["embed"].data_ptr(), w["embed"].stride(0), w["final_norm"].data_ptr()
        d.head, d.ld_head = w["head"].data_ptr(), w["head"].stride(0)
        kc = cache[0, 0]
        d.k_sb, d.k_sh, d.k_ss = kc.stride(0), kc.stride(1), kc.stride(2)
        d.v_sb, d.v_sh, d.v_ss = kc.stride(0), kc.stride(1), kc.stride(2)
        d.mask, d.mask_sb, d.position = mask8.data_ptr(), mask8.stride(0), position.data_ptr()
        d.cos, d.sin, d.rope_ld, d.rope_rows = rope[0].data_ptr(), rope[1].data_ptr(), rope[0].stride(0), rope[0].shape[0]
        d.h, d.logits, d.ld_logits = h.data_ptr(), logits.data_ptr(), logits.stride(0)
        d.finished = 0 if finished is None else finished.data_ptr()
        d.pad, d.n_eos = pad, len(eos)
        for i, e in enumerate(eos):
            d.eos[i] = e
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        return d

    def greedy_ids(self) -> Tuple[int, List[int]]:
        """``(pad, eos ids)`` as ``generate`` resolves them from the LM's generation config (no pad id: the first eos id)."""
        g = self.llm.generation_config
        eos = g.eos_token_id
        eos = [] if eos is None else [int(e) for e in (eos if isinstance(eos, (list, tuple)) else [eos])]
        if len(eos) > MAX_EOS:
            _refuse(f"at most {MAX_EOS} eos ids are taken, found {len(eos)}")
        pad = g.pad_token_id
        return int(pad if pad is not None else (eos[0] if eos else 0)), eos

    # the decode ----------------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, max_new_tokens: int, ignore_eos: bool = False,
                 keep_logits: bool = False) -> torch.Tensor:
        """What ``llm.generate(inputs_embeds=..., attention_mask=..., max_new_tokens=...)`` returns under its default greedy configuration for the
        same argmax choices: int64 [B, n] new tokens up to the step at which every sequence is finished, ``pad`` behind a sequence's eos.
        More than 8 sequences run as blocks of 8, each block to its own end (shorter blocks are filled with ``pad``).  ``ignore_eos``: no
        bookkeeping, exactly ``max_new_tokens`` tokens.  ``keep_logits``: ``self.last_logits`` [B, n, V] fp32 afterwards (tests)."""
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be at least 1")
        if not inputs_embeds.is_cuda and not self.ref:
            _refuse("generate needs CUDA tensors; there is no CPU fallback (lm_step_ref is the definition)")
        pad, eos = self.greedy_ids()
        if ignore_eos:
            eos = []
        outs, logs = [], []
        for b0 in range(0, inputs_embeds.shape[0], MAX_B):
            t, z = self._generate_block(inputs_embeds[b0:b0 + MAX_B], attention_mask[b0:b0 + MAX_B], max_new_tokens, pad, eos, keep_logits)
            outs.append(t)
            logs.append(z)
        n = max(t.shape[1] for t in outs)
        outs = [torch.cat([t, t.new_full((t.shape[0], n - t.shape[1]), pad)], 1) for t in outs]
        if keep_logits:
            self.last_logits = torch.cat([torch.cat([z, z.new_full((z.shape[0], n - z.shape[1], z.shape[2]), float("nan"))], 1) for z in logs], 0)
        return torch.cat(outs, 0)

    def _generate_block(self, embeds, mask, n_new: int, pad: int, eos: List[int], keep_logits: bool):
        llm, dev = self.llm, embeds.device
        w = walk(llm) if self.ref else self._table()[0]
        B, S0 = embeds.shape[0], embeds.shape[1]
        dt = w["head"].dtype
        mask = mask.to(dev)
        pos = mask.long().cumsum(-1) - 1                                   # generate's _prepare_position_ids_for_generation
        pos.masked_fill_(mask == 0, 1)
        was = llm.training
        llm.eval()
        try:
            with (hip_decode(llm, prefill=True) if self.prefill == "hip" else contextlib.nullcontext()):
                out = llm(inputs_embeds=embeds, attention_mask=mask, position_ids=pos, use_cache=True, return_dict=True, logits_to_keep=1)
        finally:
            llm.train(was)
        Smax = S0 + n_new
        L, Hkv, D = len(w["layers"]), w["Hkv"], w["D"]
        cache = torch.empty(L, 2, B, Hkv, Smax, D, dtype=dt, device=dev)
        for l, layer in enumerate(out.past_key_values.layers):            # the one copy of the prefill's K / V
            cache[l, 0, :, :, :S0], cache[l, 1, :, :, :S0] = layer.keys, layer.values
        mask8 = torch.ones(B, Smax, dtype=torch.uint8, device=dev)         # the bytes behind the prefix are one from the start
        mask8[:, :S0] = mask.to(torch.uint8)
        position = mask.long().sum(-1).to(torch.int32)                     # the first generated token's position; + pos_offset per step
        rope = rope_table(llm, Smax + 1, dev)
        first = out.logits[:, -1].float()
        tokens = torch.full((n_new, B), pad, dtype=torch.int32, device=dev)
        tok0, fin0 = greedy_ref(first.argmax(-1), torch.zeros(B, dtype=torch.bool, device=dev), pad, eos)
        tokens[0] = tok0.to(torch.int32)
        finished = fin0.to(torch.int32) if eos else None
        h = torch.empty(B, w["hidden"], dtype=dt, device=dev)
        logits = torch.empty(B, w["V"], dtype=torch.float32, device=dev)
        Vp = (w["V"] + 3) // 4 * 4                                         # a pitch of whole 16 bytes: every step's logits stay aligned
        kept = torch.empty(n_new, B, Vp, dtype=torch.float32, device=dev)[:, :, :w["V"]] if keep_logits else None
        if keep_logits:
            kept[0] = first
        ws = torch.empty(0 if self.ref else step_workspace_bytes(B, w["hidden"], w["inter"], w["Hq"], D, Smax), dtype=torch.uint8, device=dev)
        if not self.ref:
            d = self.descriptor(B, cache, mask8, position, rope, h, logits, finished, ws, pad, eos)
            step, stream, base, row = lib().mra_lm_step, current_stream(), tokens.data_ptr(), 4 * B
        done = n_new
        for j in range(1, n_new):
            if eos and (j - 1) % self.check_every == 0 and bool(finished.all()):       # the host's look at ``finished``
                done = j
                break
            if self.ref:
                z, _ = lm_step_ref(llm, tokens[j - 1], cache, mask8, position + (j - 1), S0 + j - 1, dtype=dt if dt != torch.float32 else None,
                                   rope=rope)
                tok, fin = greedy_ref(argmax_ref(z), finished if eos else torch.zeros(B, dtype=torch.bool, device=dev), pad, eos)
                tokens[j] = tok.to(torch.int32)
                if eos:
                    finished.copy_(fin.to(torch.int32))
                if keep_logits:
                    kept[j] = z.float()
                continue
            d.slot, d.pos_offset = S0 + j - 1, j - 1
            d.tokens_in, d.tokens_out = base + (j - 1) * row, base + j * row
            if keep_logits:
                d.logits, d.ld_logits = kept[j].data_ptr(), kept.stride(1)
            check(step(C.byref(d), stream), "mra_lm_step")
        toks = tokens[:done].T.long()
        if eos:                                                             # cut where generate stops: the step at which the last sequence finished
            hit = torch.zeros_like(toks, dtype=torch.bool)
            for e in eos:
                hit |= toks == e
            first_hit = torch.where(hit.any(1), hit.float().argmax(1), torch.full((B,), done - 1, device=dev))
            done = int(first_hit.max()) + 1
            toks = toks[:, :done]
        return toks.contiguous(), (kept[:done].transpose(0, 1).contiguous() if keep_logits else torch.empty(B, done, 0, device=dev))
