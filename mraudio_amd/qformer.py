"""Host-side mirror of the LAVIS Q-Former the reference drives, executing on the HIP extension.

Reference interface kept (``models/xinstructblip.py:286-293``)::

    out = model.video_Qformer.bert(input_ids, attention_mask=..., query_embeds=...,
                                   encoder_hidden_states=..., encoder_attention_mask=...,
                                   return_dict=True)
    out.last_hidden_state            # [N, 32 + L, 768]

``QFormer`` is an ``nn.Module`` whose parameter tree reproduces the LAVIS checkpoint key names
(``bert.embeddings.word_embeddings.weight``, ``bert.encoder.layer.{i}.attention.self.query.weight``
... reference loader ``models/xinstructblip.py:644-653``) so ``state_dict()`` /
``load_state_dict()`` / ``.to()`` behave as the reference's callers expect.  The modules are
parameter containers only: all arithmetic happens in ``libmra_hip.so``; torch provides device
memory and the stream.  There is no CPU path.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import weakref
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib
from ._lib import MRA_BF16, MRA_F16, MRA_F32, MraError, check, current_stream, lib, mra_cfg, ptr


@dataclass
class QFormerConfig:
    """BERT-base + cross-attention every 2nd layer (reference ``models/xinstructblip.py:614-627``)."""

    hidden: int = 768
    heads: int = 12
    inter: int = 3072
    layers: int = 12
    cross_freq: int = 2
    enc_width: int = 1408
    n_query: int = 32
    vocab: int = 30523
    max_pos: int = 512
    ln_eps: float = 1e-12
    enc_ln_eps: float = 1e-5
    llm_hidden: int = 4096
    op_dtype: torch.dtype = torch.float16  # MFMA operand type; accumulation/residual/LN stay fp32

    def to_c(self) -> mra_cfg:
        return mra_cfg(self.hidden, self.heads, self.inter, self.layers, self.cross_freq, self.enc_width, self.n_query,
                       self.vocab, self.max_pos, self.ln_eps, self.enc_ln_eps, self.llm_hidden,
                       MRA_BF16 if self.op_dtype == torch.bfloat16 else MRA_F16)


CROSS_MODES = {"auto": 0, "kv_cache": 1, "fold": 2, "fold384": 3, "fold_stream": 4, "fold_rescale_pass": 5}   # mra_qformer_set_cross_mode


def _check_pushed(what: str, pairs, pushed: dict) -> None:
    """``MraError`` unless every ``(name, tensor)`` of ``pairs`` is the tensor last pushed to the handle under ``name``, at the version it
    was pushed at (``pushed[name]`` = (weak reference, version)).  ``what``: the calling method, for the message."""
    for name, t in pairs:
        ref, ver = pushed.get(name, (None, None))
        if ref is None or ref() is not t:
            raise MraError(f"{what}: {name} is not the tensor last pushed to the handle (push it first)")
        if ver != t._version:
            raise MraError(f"{what}: {name} changed since it was pushed (version {ver} -> {t._version}): push it again")


@contextlib.contextmanager
def _kv_events(handle, events):
    """While the block runs, the library records the (start, stop) ``torch.cuda.Event`` pair ``events`` around the handle's dominant
    kernel on the launch stream (``mra_qformer_set_kv_events``); cleared again on the way out, also after an error.  ``None``: nothing."""
    if events is None:
        yield
        return
    check(lib().mra_qformer_set_kv_events(handle, events[0].cuda_event, events[1].cuda_event), "set_kv_events")
    try:
        yield
    finally:
        check(lib().mra_qformer_set_kv_events(handle, None, None), "set_kv_events")


class _Lin(nn.Module):
    def __init__(self, out_f: int, in_f: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_f, in_f), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_f), requires_grad=False)


class _LN(nn.Module):
    def __init__(self, n: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(n), requires_grad=False)


class _Emb(nn.Module):
    def __init__(self, n: int, d: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(n, d), requires_grad=False)


class _Wrap(nn.Module):
    def __init__(self, **children):
        super().__init__()
        for k, v in children.items():
            self.add_module(k, v)


def _attention(h: int, kv_width: int) -> nn.Module:
    self_ = _Wrap(query=_Lin(h, h), key=_Lin(h, kv_width), value=_Lin(h, kv_width))
    out = _Wrap(dense=_Lin(h, h), LayerNorm=_LN(h))
    m = nn.Module()
    m.add_module("self", self_)
    m.add_module("output", out)
    return m


class _Bert(nn.Module):
    """``qformer.bert``: parameter container named like LAVIS' ``BertModel`` whose call signature is
    the one the reference uses (``models/xinstructblip.py:286-293``)."""

    def __init__(self, embeddings: nn.Module, encoder: nn.Module):
        super().__init__()
        self.embeddings = embeddings
        self.encoder = encoder
        object.__setattr__(self, "_owner_ref", None)

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, query_embeds=None,
                encoder_hidden_states=None, encoder_attention_mask=None, return_dict=True, **unused):
        o = self._owner_ref()
        if encoder_hidden_states is None:
            raise ValueError("encoder_hidden_states must be given for cross-attention layers")
        if query_embeds is None:
            raise ValueError("You have to specify query_embeds")
        if position_ids is not None:
            raise NotImplementedError("custom position_ids are not supported (the reference never passes them)")
        if encoder_attention_mask is not None and not bool(encoder_attention_mask.to(torch.bool).all()):
            raise NotImplementedError("encoder_attention_mask with zeros is not supported: the reference always "
                                      "passes all ones (models/xinstructblip.py:266,275)")
        res = o.forward_fused(input_ids, attention_mask, encoder_hidden_states, query_embeds=query_embeds,
                              want_query=False, want_full=True)
        out = QFormerOutput(res["full"])
        return out if return_dict else (out.last_hidden_state,)


def _bert_tree(cfg: QFormerConfig) -> "_Bert":
    emb = _Wrap(word_embeddings=_Emb(cfg.vocab, cfg.hidden), position_embeddings=_Emb(cfg.max_pos, cfg.hidden),
                LayerNorm=_LN(cfg.hidden))
    layers = nn.ModuleList()
    for i in range(cfg.layers):
        lay = nn.Module()
        lay.add_module("attention", _attention(cfg.hidden, cfg.hidden))
        if i % cfg.cross_freq == 0:
            lay.add_module("crossattention", _attention(cfg.hidden, cfg.enc_width))
        lay.add_module("intermediate", _Wrap(dense=_Lin(cfg.inter, cfg.hidden)))
        lay.add_module("output", _Wrap(dense=_Lin(cfg.hidden, cfg.inter), LayerNorm=_LN(cfg.hidden)))
        lay.add_module("intermediate_query", _Wrap(dense=_Lin(cfg.inter, cfg.hidden)))
        lay.add_module("output_query", _Wrap(dense=_Lin(cfg.hidden, cfg.inter), LayerNorm=_LN(cfg.hidden)))
        layers.append(lay)
    return _Bert(emb, _Wrap(layer=layers))


def seeded_parameter_order(cfg: QFormerConfig) -> List[Tuple[str, str]]:
    """(key, kind) in the order the seeded synthetic init draws tensors; kind in w/b/g/z
    (matrix, bias, LayerNorm gain, LayerNorm bias).  Same order as the checker's recipe."""
    out = [("bert.embeddings.word_embeddings.weight", "w"), ("bert.embeddings.position_embeddings.weight", "w"),
           ("bert.embeddings.LayerNorm.weight", "g"), ("bert.embeddings.LayerNorm.bias", "z")]
    for i in range(cfg.layers):
        p = f"bert.encoder.layer.{i}."
        blocks = ["attention"] + (["crossattention"] if i % cfg.cross_freq == 0 else [])
        for blk in blocks:
            for n in ("query", "key", "value"):
                out += [(p + f"{blk}.self.{n}.weight", "w"), (p + f"{blk}.self.{n}.bias", "b")]
            out += [(p + f"{blk}.output.dense.weight", "w"), (p + f"{blk}.output.dense.bias", "b"),
                    (p + f"{blk}.output.LayerNorm.weight", "g"), (p + f"{blk}.output.LayerNorm.bias", "z")]
        for suf in ("", "_query"):
            out += [(p + f"intermediate{suf}.dense.weight", "w"), (p + f"intermediate{suf}.dense.bias", "b"),
                    (p + f"output{suf}.dense.weight", "w"), (p + f"output{suf}.dense.bias", "b"),
                    (p + f"output{suf}.LayerNorm.weight", "g"), (p + f"output{suf}.LayerNorm.bias", "z")]
    return out


def draw_seeded(gen: torch.Generator, shape, kind: str, perturb: bool) -> torch.Tensor:
    """One tensor of the synthetic init: matrices N(0, 0.02) (``initializer_range``, reference
    ``models/xinstructblip.py:627``); biases 0, LayerNorm 1/0 -- or, with ``perturb``, biases
    N(0, 0.02), gains 1 + N(0, 0.1), LayerNorm biases N(0, 0.05) so every parameter matters."""
    if kind == "w":
        return torch.randn(shape, generator=gen, dtype=torch.float32) * 0.02
    if kind == "b":
        return torch.randn(shape, generator=gen) * 0.02 if perturb else torch.zeros(shape)
    if kind == "g":
        return 1.0 + torch.randn(shape, generator=gen) * 0.1 if perturb else torch.ones(shape)
    return torch.randn(shape, generator=gen) * 0.05 if perturb else torch.zeros(shape)


class QFormerOutput:
    """What the reference reads from the LAVIS model output (``.last_hidden_state``, ``:303``)."""

    def __init__(self, last_hidden_state: torch.Tensor):
        self.last_hidden_state = last_hidden_state
        self.pooler_output = None

    def __getitem__(self, i):
        return (self.last_hidden_state,)[i]


class QFormer(nn.Module):
    """One modality Q-Former on one GPU (one ``mra_qformer`` handle)."""

    def __init__(self, cfg: QFormerConfig, device: Optional[torch.device] = None):
        super().__init__()
        self.cfg = cfg
        self.bert = _bert_tree(cfg)
        object.__setattr__(self.bert, "_owner_ref", weakref.ref(self))
        self._handle = C.c_void_p()
        self._device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._ws: Optional[torch.Tensor] = None
        self._dirty = True
        with torch.cuda.device(self._device):
            c = cfg.to_c()
            check(lib().mra_qformer_create(C.byref(c), C.byref(self._handle)), "mra_qformer_create")
        self.bert.to(self._device)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        # LAVIS checkpoints also carry the position_ids buffer and the LM head the reference deletes
        # (``modality_qformer.cls = None``, models/xinstructblip.py:135)
        sd = {k: v for k, v in state_dict.items() if k != "bert.embeddings.position_ids" and not k.startswith("cls.")}
        res = super().load_state_dict(sd, strict=strict, assign=assign)
        self._dirty = True
        return res

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._dirty = True
        return out

    def __del__(self):
        try:
            if self._handle:
                lib().mra_qformer_destroy(self._handle)
                self._handle = C.c_void_p()
        except Exception:
            pass

    # ---- weights -> handle ---------------------------------------------------------------------
    def push(self, name: str, t: torch.Tensor) -> None:
        """Copy one tensor into the handle under its ABI name (``include/mra.h`` mra_qformer_load)."""
        if name in ("ln.weight", "ln.bias"):      # modality_ln_train checks that it is handed the tensors the handle holds
            self.__dict__.setdefault("_pushed_ln", {})[name] = (weakref.ref(t), t._version)
        if name in ("llm_proj.weight", "llm_proj.bias"):      # likewise llm_proj_train
            self.__dict__.setdefault("_pushed_proj", {})[name] = (weakref.ref(t), t._version)
        t = t.detach()
        if t.device != self._device:
            t = t.to(self._device)
        if t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            t = t.float()
        t = t.contiguous()
        shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
        with torch.cuda.device(self._device):
            check(lib().mra_qformer_load(self._handle, name.encode(), ptr(t), _lib.mra_dtype(t.dtype), shape, t.dim(),
                                         current_stream()), f"mra_qformer_load({name})")

    def sync_weights(self) -> None:
        # in-place updates (an optimizer step) bump the tensors' version counters
        ver = sum(p._version for p in self.bert.parameters())
        if ver != getattr(self, "_param_version", None):
            self._param_version = ver
            self._dirty = True
        if not self._dirty:
            return
        if getattr(self, "_master_flat", None) is not None:
            # training: the parameters are views of one flat f32 master buffer -> one launch refreshes all
            self._bind_master()
            with torch.cuda.device(self._device):
                check(lib().mra_qformer_load_flat(self._handle, ptr(self._master_flat), self._master_flat.numel() * 4, current_stream()),
                      "mra_qformer_load_flat")
        else:
            for k, v in self.bert.state_dict(prefix="bert.").items():
                self.push(k, v)
        self._dirty = False

    def missing(self) -> List[str]:
        buf = C.create_string_buffer(1 << 16)
        n = lib().mra_qformer_missing(self._handle, buf, len(buf))
        return [s for s in buf.value.decode().split(",") if s] if n else []

    @torch.no_grad()
    def init_seeded_(self, seed: int = 0, perturb: bool = False, gen: Optional[torch.Generator] = None) -> torch.Generator:
        """Synthetic weights (no pretrained checkpoints exist offline).  Drawn on the CPU from one
        generator in ``seeded_parameter_order`` so that every machine derives the same tensors."""
        g = gen if gen is not None else torch.Generator().manual_seed(seed)
        sd = self.bert.state_dict(prefix="bert.", keep_vars=True)
        for key, kind in seeded_parameter_order(self.cfg):
            p = sd[key]
            p.data.copy_(draw_seeded(g, tuple(p.shape), kind, perturb))
        self._dirty = True
        return g

    # ---- ops -----------------------------------------------------------------------------------
    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self._device)
        return self._ws

    def modality_ln(self, x: torch.Tensor, item_index: Optional[torch.Tensor] = None, items: Optional[int] = None) -> torch.Tensor:
        """A2 + A3: ``ln(encoder(frame))`` then ``cat(embeds)[indices]`` (reference ``:265,281-285``).
        x [src_items, tokens, E] f32/f16/bf16 -> [items, tokens, E] operand dtype."""
        if x.dim() != 3 or x.shape[-1] != self.cfg.enc_width:
            raise MraError(f"modality_ln expects [items, tokens, {self.cfg.enc_width}], got {tuple(x.shape)}")
        x = x.contiguous()
        n = int(items if items is not None else (item_index.numel() if item_index is not None else x.shape[0]))
        if item_index is not None:
            item_index = item_index.to(device=x.device, dtype=torch.int64).contiguous()
        out = torch.empty((n, x.shape[1], x.shape[2]), dtype=self.cfg.op_dtype, device=x.device)
        with torch.cuda.device(self._device):
            check(lib().mra_modality_ln(self._handle, ptr(x), _lib.mra_dtype(x.dtype), ptr(item_index), n, x.shape[1],
                                        ptr(out), current_stream()), "mra_modality_ln")
        return out

    def modality_ln_train(self, x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
        """``modality_ln(x)`` (identity item order, the same bits) connected to autograd: ``weight`` / ``bias`` are the ``{m}_ln``
        tensors last pushed as ``ln.weight`` / ``ln.bias`` -- ordinary torch parameters, not slots of the flat buffer -- and receive
        real ``.grad`` tensors from ``mra_modality_ln_backward``; ``x`` [items, tokens, E] receives one only if it requires grad.
        ``MraError`` if the handle holds other tensors (or an older version of these) than the ones given."""
        _check_pushed("modality_ln_train", (("ln.weight", weight), ("ln.bias", bias)), getattr(self, "_pushed_ln", {}))
        return _ModalityLNTrainFn.apply(x, weight, bias, self)

    def _ln_backward(self, x: torch.Tensor, d_out: torch.Tensor, want_x: bool, want_gain: bool, want_bias: bool):
        """``mra_modality_ln_backward`` over raw features x [items, tokens, E] and the fp32 upstream gradient: (d_x or None -- written
        over ``d_out`` in place --, d_gain or None, d_bias or None), fp32."""
        E = self.cfg.enc_width
        d_gain = torch.zeros(E, dtype=torch.float32, device=x.device) if want_gain else None
        d_bias = torch.zeros(E, dtype=torch.float32, device=x.device) if want_bias else None
        with torch.cuda.device(self._device):
            check(lib().mra_modality_ln_backward(self._handle, ptr(x), _lib.mra_dtype(x.dtype), int(x.shape[0]), int(x.shape[1]), ptr(d_out),
                                                 ptr(d_out) if want_x else None, ptr(d_gain), ptr(d_bias), current_stream()),
                  "mra_modality_ln_backward")
        return (d_out if want_x else None), d_gain, d_bias

    def raw_features_ok(self, x: torch.Tensor, item_index: Optional[torch.Tensor] = None) -> bool:
        """Can ``forward_fused(..., raw=True)`` read the encoder output ``x`` [N, Kv, E] itself, with no ``modality_ln`` pass
        (``mra_qformer_raw_features_ok``)?  Contiguous features in the operand dtype on the handle's device, no item gather, and a form
        the library folds the LayerNorm into."""
        if item_index is not None or x.dim() != 3 or x.shape[-1] != self.cfg.enc_width or x.dtype != self.cfg.op_dtype or not x.is_contiguous():
            return False
        if x.shape[0] == 0 or x.device != self._device:
            return False
        self.sync_weights()
        return bool(lib().mra_qformer_raw_features_ok(self._handle, int(x.shape[1]), _lib.mra_dtype(x.dtype)))

    def _prepare(self, input_ids, attention_mask, enc, prompts: int = 1):
        """What every forward checks and casts before it calls the library: enc [N, Kv, E] to the operand dtype, contiguous; input_ids
        [N * prompts, L] and attention_mask [N * prompts, 32 + L] to int64 on enc's device.  ``MraError`` on any other shape (the kernels
        index by these sizes).  Returns ``(input_ids, attention_mask, enc, N, L, Kv)``."""
        cfg = self.cfg
        if enc.dim() != 3 or enc.shape[-1] != cfg.enc_width:
            raise MraError(f"encoder_hidden_states must be [N, Kv, {cfg.enc_width}], got {tuple(enc.shape)}")
        enc = enc.to(cfg.op_dtype).contiguous()
        N, Kv = int(enc.shape[0]), int(enc.shape[1])
        rows = N * prompts
        L = 0
        if input_ids is not None:
            if input_ids.shape[0] != rows:
                raise MraError(f"input_ids has {input_ids.shape[0]} rows, encoder_hidden_states {N}" + (f" x prompts {prompts}" if prompts != 1 else ""))
            L = int(input_ids.shape[1])
            input_ids = input_ids.to(device=enc.device, dtype=torch.int64).contiguous()
        if attention_mask is not None:
            if tuple(attention_mask.shape) != (rows, cfg.n_query + L):
                raise MraError(f"attention_mask must be [{rows}, {cfg.n_query + L}], got {tuple(attention_mask.shape)}")
            attention_mask = attention_mask.to(device=enc.device, dtype=torch.int64).contiguous()
        return input_ids, attention_mask, enc, N, L, Kv

    def forward_fused(self, input_ids: Optional[torch.Tensor], attention_mask: Optional[torch.Tensor], enc: torch.Tensor,
                      query_embeds: Optional[torch.Tensor] = None, want_query: bool = True, want_full: bool = False,
                      want_cls: bool = False, kv_events=None, raw: bool = False) -> Dict[str, torch.Tensor]:
        """A4 on the extension.  enc [N, Kv, E] in the operand dtype (``modality_ln`` output; with ``raw`` the encoder output itself,
        where ``raw_features_ok`` allows it: ``mra_qformer_forward_raw``).
        Returns a dict with ``query`` [N,32,H], ``full`` [N,32+L,H], ``cls`` [N,H] (fp32) as requested.
        ``kv_events``: optional (start, stop) ``torch.cuda.Event`` pair for ``_kv_events`` (bench
        instrumentation of the dominant kernel, recorded by the library on the launch stream)."""
        self.sync_weights()
        cfg = self.cfg
        if raw and (enc.dtype != cfg.op_dtype or not enc.is_contiguous()):
            raise MraError("raw features must be contiguous and in the operand dtype (ask raw_features_ok)")
        input_ids, attention_mask, enc, N, L, Kv = self._prepare(input_ids, attention_mask, enc)
        dev = enc.device
        q_items = 0
        if query_embeds is not None:
            if query_embeds.dim() != 3 or tuple(query_embeds.shape[1:]) != (cfg.n_query, cfg.hidden) or query_embeds.shape[0] not in (1, N):
                raise MraError(f"query_embeds must be [1 or {N}, {cfg.n_query}, {cfg.hidden}]")
            query_embeds = query_embeds.to(device=dev, dtype=torch.float32).contiguous()
            q_items = int(query_embeds.shape[0])
        out: Dict[str, torch.Tensor] = {}
        if N == 0:
            return {"query": torch.empty(0, cfg.n_query, cfg.hidden, device=dev), "full": torch.empty(0, cfg.n_query + L, cfg.hidden, device=dev),
                    "cls": torch.empty(0, cfg.hidden, device=dev)}
        if want_query:
            out["query"] = torch.empty(N, cfg.n_query, cfg.hidden, dtype=torch.float32, device=dev)
        if want_full:
            out["full"] = torch.empty(N, cfg.n_query + L, cfg.hidden, dtype=torch.float32, device=dev)
        if want_cls:
            out["cls"] = torch.empty(N, cfg.hidden, dtype=torch.float32, device=dev)
        with torch.cuda.device(self._device):
            nbytes = (int(lib().mra_qformer_workspace_bytes(self._handle, N, L, Kv)) + 255) // 256 * 256
            ws = self._workspace(nbytes)
            with _kv_events(self._handle, kv_events):
                fwd = lib().mra_qformer_forward_raw if raw else lib().mra_qformer_forward
                check(fwd(
                    self._handle, ptr(input_ids), ptr(attention_mask), ptr(query_embeds), q_items, ptr(enc), N, L, Kv,
                    ptr(out.get("query")), ptr(out.get("full")), ptr(out.get("cls")), ptr(ws), nbytes, current_stream()),
                    "mra_qformer_forward_raw" if raw else "mra_qformer_forward")
        return out

    def forward_multi(self, input_ids: Optional[torch.Tensor], attention_mask: Optional[torch.Tensor], enc: torch.Tensor, prompts: int,
                      want_query: bool = True, want_cls: bool = False) -> Dict[str, torch.Tensor]:
        """``prompts`` prompts per encoder item over one shared K/V cache (``mra_qformer_forward_multi``).  enc [N, Kv, E] in the
        operand dtype, given once per item; row ``i * prompts + p`` of ``input_ids`` [N * prompts, L] and ``attention_mask``
        [N * prompts, 32 + L] is prompt slot ``p`` of item ``i``.  Returns ``query`` [N * prompts, 32, H] and / or ``cls``
        [N * prompts, H] (fp32) in the same row order.  Always the K/V-cache form in operand precision (``MraError`` while split
        precision is in force or automatic precision has not resolved to op); ``prompts == 1`` is ``forward_fused`` under
        ``set_cross_mode("kv_cache")``.  The cross core follows ``set_option("multi_core", 0 / 1)``."""
        self.sync_weights()
        cfg = self.cfg
        P = int(prompts)
        if P < 1:
            raise MraError(f"prompts must be >= 1, got {prompts}")
        input_ids, attention_mask, enc, N, L, Kv = self._prepare(input_ids, attention_mask, enc, P)
        dev = enc.device
        if N == 0:
            return {"query": torch.empty(0, cfg.n_query, cfg.hidden, device=dev), "cls": torch.empty(0, cfg.hidden, device=dev)}
        out: Dict[str, torch.Tensor] = {}
        if want_query:
            out["query"] = torch.empty(N * P, cfg.n_query, cfg.hidden, dtype=torch.float32, device=dev)
        if want_cls:
            out["cls"] = torch.empty(N * P, cfg.hidden, dtype=torch.float32, device=dev)
        with torch.cuda.device(self._device):
            nbytes = (int(lib().mra_qformer_multi_workspace_bytes(self._handle, N, P, L, Kv)) + 255) // 256 * 256
            ws = self._workspace(nbytes)
            check(lib().mra_qformer_forward_multi(self._handle, ptr(input_ids), ptr(attention_mask), ptr(enc), N, P, L, Kv,
                                                  ptr(out.get("query")), ptr(out.get("cls")), ptr(ws), nbytes, current_stream()),
                  "mra_qformer_forward_multi")
        return out

    @staticmethod
    def forward_pair(qf0: "QFormer", qf1: "QFormer", input_ids: Optional[torch.Tensor], attention_mask: Optional[torch.Tensor], enc0: torch.Tensor,
                     enc1: torch.Tensor, want_cls: bool = True, kv_events=None, raw=(False, False)):
        """Both modality Q-Formers of a step in ONE launch sequence (``mra_qformer_forward_pair``): the layer chains as grouped launches,
        each lane its own cross-attention.  enc0 / enc1 [N, Kv_l, E_l] in the operand dtype, the same prompt rows for both lanes.  Returns
        ``[(query0, cls0), (query1, cls1)]`` (fp32; cls ``None`` without ``want_cls``).  ``kv_events``: (start, stop) pair for lane 0's
        cross-layer-0 block (bench instrumentation).  ``raw[l]``: lane l's enc is the encoder output itself (``raw_features_ok``;
        ``mra_qformer_forward_pair_raw``)."""
        qfs = (qf0, qf1)
        for qf in qfs:
            qf.sync_weights()
        input_ids, attention_mask, enc0, N, L, _ = qf0._prepare(input_ids, attention_mask, enc0)
        encs = [enc0, qf1._prepare(None, None, enc1)[2]]
        if int(encs[1].shape[0]) != N:
            raise MraError("forward_pair: both lanes need the same number of items")
        dev = enc0.device
        H, Q = qf0.cfg.hidden, qf0.cfg.n_query
        outs = [(torch.empty(N, Q, H, dtype=torch.float32, device=dev), torch.empty(N, H, dtype=torch.float32, device=dev) if want_cls else None) for _ in qfs]
        if N == 0:
            return outs
        with torch.cuda.device(qf0._device):
            nbytes = (int(lib().mra_qformer_pair_workspace_bytes(qf0._handle, qf1._handle, N, L, int(encs[0].shape[1]), int(encs[1].shape[1]))) + 255) // 256 * 256
            ws = qf0._workspace(nbytes)
            with _kv_events(qf0._handle, kv_events):
                check(lib().mra_qformer_forward_pair_raw(qf0._handle, qf1._handle, ptr(input_ids), ptr(attention_mask), ptr(encs[0]), ptr(encs[1]),
                                                         int(bool(raw[0])) | int(bool(raw[1])) << 1, N, L,
                                                         int(encs[0].shape[1]), int(encs[1].shape[1]), ptr(outs[0][0]), ptr(outs[0][1]), ptr(outs[1][0]), ptr(outs[1][1]),
                                                         ptr(ws), nbytes, current_stream()), "mra_qformer_forward_pair")
        return outs

    def llm_proj(self, z: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """A5: ``{modality}_llm_proj(last_hidden_state[:, :32, :])`` (reference ``:303``)."""
        cfg = self.cfg
        zz = z.reshape(-1, cfg.hidden).to(torch.float32).contiguous()
        rows = int(zz.shape[0])
        out = torch.empty(rows, cfg.llm_hidden, dtype=out_dtype, device=zz.device)
        ws = self._workspace(max(256, rows * cfg.hidden * 2 + 256))
        with torch.cuda.device(self._device):
            check(lib().mra_llm_proj(self._handle, ptr(zz), rows, ptr(out), _lib.mra_dtype(out_dtype), ptr(ws), ws.numel(),
                                     current_stream()), "mra_llm_proj")
        return out.reshape(*z.shape[:-1], cfg.llm_hidden)

    def llm_proj_train(self, z: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, out_dtype: torch.dtype = torch.float32,
                       grad_scale: float = 1.0) -> torch.Tensor:
        """``llm_proj(z, out_dtype)`` (the same bits) connected to autograd: ``weight`` / ``bias`` are the ``{m}_llm_proj`` tensors last
        pushed as ``llm_proj.weight`` / ``llm_proj.bias`` -- ordinary torch parameters, not slots of the flat buffer -- and receive real
        ``.grad`` tensors from ``mra_llm_proj_backward`` if they require one; ``z`` receives its gradient if it requires one (the output of
        ``forward_train`` does).  ``MraError`` if the handle holds other tensors (or an older version of these) than the ones given.
        ``grad_scale``: the upstream gradient arrives multiplied by it (a loss scale that keeps a 16-bit LM's gradients out of the
        underflow range) and is divided by it in fp32 before the backward runs, so every gradient this node hands on is unscaled."""
        _check_pushed("llm_proj_train", (("llm_proj.weight", weight), ("llm_proj.bias", bias)), getattr(self, "_pushed_proj", {}))
        return _LlmProjTrainFn.apply(z, weight, bias, self, out_dtype, float(grad_scale))

    def _proj_backward(self, z: torch.Tensor, d_out: torch.Tensor, want_z: bool, want_w: bool, want_b: bool):
        """One ``mra_llm_proj_backward`` over z [rows, H] fp32 and d_out [rows, llm_hidden] (fp32 or the operand dtype): (d_z or None,
        d_weight or None, d_bias or None), fp32, the parameter gradients fresh zeroed buffers the entry added to."""
        cfg = self.cfg
        rows, dev = int(z.shape[0]), z.device
        d_z = torch.empty(rows, cfg.hidden, dtype=torch.float32, device=dev) if want_z else None
        d_w = torch.zeros(cfg.llm_hidden, cfg.hidden, dtype=torch.float32, device=dev) if want_w else None
        d_b = torch.zeros(cfg.llm_hidden, dtype=torch.float32, device=dev) if want_b else None
        with torch.cuda.device(self._device):
            dt = _lib.mra_dtype(d_out.dtype)
            nbytes = int(lib().mra_llm_proj_backward_workspace_bytes(self._handle, rows, dt))
            ws = self._workspace(max(256, nbytes))
            check(lib().mra_llm_proj_backward(self._handle, ptr(z), rows, ptr(d_out), dt, ptr(d_z), ptr(d_w), ptr(d_b), ptr(ws), ws.numel(),
                                              current_stream()), "mra_llm_proj_backward")
        return d_z, d_w, d_b

    def set_cross_mode(self, mode) -> None:
        """How the cross-attention layers run: ``"auto"`` (folded from Kv >= 2048), ``"kv_cache"``, ``"fold"``, or the
        A/B formulations ``"fold384"`` (128 x 384 tiles) / ``"fold_stream"`` (streaming kernels, f16 only)
        (``mra_qformer_set_cross_mode``).  Same arithmetic, re-associated; the workspace size follows the mode."""
        code = CROSS_MODES.get(mode, mode)
        check(lib().mra_qformer_set_cross_mode(self._handle, int(code)), "mra_qformer_set_cross_mode")
        self._cross_mode = mode if isinstance(mode, str) else {v: k for k, v in CROSS_MODES.items()}.get(int(mode), "auto")

    def set_option(self, name: str, value: int) -> None:
        """Per-handle tuning option (``mra_qformer_set_option``), e.g. ``("chain_ring", mask)``."""
        check(lib().mra_qformer_set_option(self._handle, name.encode(), int(value)), f"mra_qformer_set_option({name})")

    def set_cross_precision(self, mode) -> None:
        """Precision of the cross-attention score chain: ``"op"`` (default: f16 / bf16 operands), ``"split"`` (hidden state, W_cq, Q,
        W_k and Q' as hi + lo pairs, ~22 bits; folded form at any Kv) or ``"auto"`` (``mra_qformer_set_cross_precision``).  Split is
        for sharply attending (trained) weights, where the f16 rounding of the score operands is amplified by the softmax; auto measures
        how peaked the attention is on the first forward after every weight upload (one host sync on that call) and runs split iff the
        largest per-cross-layer median softmax row maximum reaches the threshold (0.5; option ``auto_split_pmax_milli``), op otherwise.
        The workspace size follows the mode (under auto: the largest of the forms the handle may run)."""
        code = {"op": 0, "f16": 0, "split": 1, "auto": 2}.get(mode, mode)
        with torch.cuda.device(self._device):
            check(lib().mra_qformer_set_cross_precision(self._handle, int(code)), "mra_qformer_set_cross_precision")
        self._cross_precision = {0: "op", 1: "split", 2: "auto"}[int(code)]

    def cross_precision_report(self) -> Dict[str, object]:
        """``{"mode", "resolved", "probes", "median_pmax"}``: the mode set (``"op"`` / ``"split"`` / ``"auto"``), the precision in force
        (``"op"`` / ``"split"``, ``None`` while an auto probe is pending), the number of auto probes since the handle was created and,
        per cross layer, the median softmax row maximum of the last probe (-1 before any; ``mra_qformer_cross_precision_report``)."""
        ncross = -(-self.cfg.layers // self.cfg.cross_freq) if self.cfg.cross_freq > 0 else 0   # layers i with i % cross_freq == 0
        resolved, probes = C.c_int32(), C.c_int32()
        med = (C.c_float * max(1, ncross))()
        check(lib().mra_qformer_cross_precision_report(self._handle, C.byref(resolved), C.byref(probes), med, max(1, ncross)),
              "mra_qformer_cross_precision_report")
        return {"mode": getattr(self, "_cross_precision", "op"), "resolved": {0: "op", 1: "split"}.get(int(resolved.value)),
                "probes": int(probes.value), "median_pmax": [float(med[i]) for i in range(ncross)]}

    def flops(self, items: int, L: int, kv: int, with_last_text: bool) -> float:
        return float(lib().mra_qformer_flops(self._handle, items, L, kv, int(with_last_text)))

    # ---- training (BASELINE config 5): forward with an activation tape + HIP backward behind torch.autograd ----
    def enable_training(self) -> None:
        """Allocate the flat gradient buffer, bind every ``bert.*`` parameter's ``.grad`` to its slice and build
        the transposed weight copies (call again after changing weights; ``forward_train`` does it lazily)."""
        self.sync_weights()
        with torch.cuda.device(self._device):
            check(lib().mra_qformer_enable_training(self._handle, current_stream()), "mra_qformer_enable_training")
        if getattr(self, "_grad_flat", None) is None:
            n = int(lib().mra_qformer_grad_bytes(self._handle)) // 4
            self._grad_flat = torch.zeros(n, dtype=torch.float32, device=self._device)
            self._anchor = torch.zeros((), dtype=torch.float32, device=self._device, requires_grad=True)
            self._train_ws = None       # the spare tape buffer: the one a training node took last, handed back after its backward
            self._slices = {}
            for k, p in self.bert.state_dict(prefix="bert.", keep_vars=True).items():
                self._slices[k] = (*self._slice_of(k), p)
                p.requires_grad_(True)
            # master weights: one flat f32 buffer in the gradient buffer's layout; every parameter becomes a view of
            # it, so any optimizer updates it in place and mra_qformer_load_flat refreshes the device copies at once
            self._master_flat = torch.zeros(n, dtype=torch.float32, device=self._device)
            self._bind_master()


    def _bind_master(self) -> None:
        """(Re-)point every ``bert.*`` parameter at its slice of the master buffer.  ``module.to()`` /
        ``load_state_dict(assign=True)`` replace parameter storage; the current values are carried over."""
        base = self._master_flat.data_ptr()
        first = next(iter(self._slices.values()))
        if first[2].data_ptr() == base + first[0] * 4 and getattr(self, "_master_bound", False):
            return
        with torch.no_grad():
            for off, numel, p in self._slices.values():
                view = self._master_flat[off: off + numel].view(p.shape)
                if p.data_ptr() != view.data_ptr():
                    view.copy_(p.data)
                    p.data = view
        self._master_bound = True


    def grad_of(self, name: str) -> torch.Tensor:
        """View of parameter ``name``'s gradient inside the flat buffer (ABI names, e.g. ``query_tokens``)."""
        off, numel = C.c_size_t(), C.c_int64()
        check(lib().mra_qformer_grad_offset(self._handle, name.encode(), C.byref(off), C.byref(numel)), f"grad_offset({name})")
        return self._grad_flat[off.value // 4: off.value // 4 + numel.value]


    def _bind_grads(self) -> None:
        probe = self.bert.embeddings.LayerNorm.weight
        if probe.grad is not None and probe.grad.data_ptr() == self.grad_of("bert.embeddings.LayerNorm.weight").data_ptr():
            return                                   # still bound from the previous backward
        for off, numel, p in self._slices.values():
            p.grad = self._grad_flat[off: off + numel].view(p.shape)


    def forward_train(self, input_ids, attention_mask, enc, want_cls: bool = True):
        """Training forward: ``(out_query [N,32,H], out_cls [N,H])`` connected to autograd.  ``loss.backward()``
        accumulates parameter gradients (``p.grad`` of every ``bert.*`` parameter, ``grad_of('query_tokens')``).
        ``forward_multi_train`` with one prompt per item; ``MraError`` on zero items."""
        if enc.dim() == 3 and enc.shape[0] == 0:
            raise MraError("forward_train: no items")
        return self.forward_multi_train(input_ids, attention_mask, enc, 1, want_cls)


    def forward_multi_train(self, input_ids, attention_mask, enc, prompts: int, want_cls: bool = True):
        """Training forward for ``prompts`` prompts per encoder item over one shared K/V cache (``mra_qformer_forward_multi_train``):
        ``(out_query [N * prompts, 32, H], out_cls [N * prompts, H])`` connected to autograd, row ``i * prompts + p`` = item ``i``,
        prompt slot ``p`` (the row order of ``forward_multi``).  enc [N, Kv, E] is given once per item.  Equal to ``forward_train`` on
        ``enc.repeat_interleave(prompts, 0)``; the K/V projection, the dK / dV tape and the K/V weight gradients run once per item.
        ``loss.backward()`` accumulates gradients into the flat buffer.  ``prompts`` is limited by the LDS of the attention backward
        (14 at 32 query tokens; ``MraError`` beyond).  Every call's node holds its tape until its backward has run, so several
        forwards may precede their backwards, in any order."""
        self.enable_training()
        P = int(prompts)
        if P < 1:
            raise MraError(f"prompts must be >= 1, got {prompts}")
        input_ids, attention_mask, enc, _, _, _ = self._prepare(input_ids, attention_mask, enc, P)
        q, c = _QFormerTrainFn.apply(self._anchor, self, input_ids, attention_mask, enc, P, want_cls)
        return (q, c) if want_cls else (q, None)


    def _slice_of(self, name: str):
        off, numel = C.c_size_t(), C.c_int64()
        check(lib().mra_qformer_grad_offset(self._handle, name.encode(), C.byref(off), C.byref(numel)), f"grad_offset({name})")
        return off.value // 4, int(numel.value)


    def flat_parameter(self) -> torch.nn.Parameter:
        """ONE ``nn.Parameter`` over the whole master buffer with the whole gradient buffer as its ``.grad``: an
        optimizer given this instead of the ~400 per-tensor parameters updates the Q-Former in one fused launch
        (fused Adam over 186 M elements: 0.8 ms instead of 2.3 ms for the per-tensor lists).  The per-tensor
        parameters stay valid views of the same memory (state_dict, checkpoints)."""
        self.enable_training()
        fp = getattr(self, "_flat_param", None)
        if fp is None or fp.data_ptr() != self._master_flat.data_ptr():
            fp = torch.nn.Parameter(self._master_flat, requires_grad=True)
            object.__setattr__(self, "_flat_param", fp)      # not registered: it aliases the per-tensor parameters
        fp.grad = self._grad_flat
        return fp


    def adam_step(self, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, zero_grad: bool = True) -> None:
        """One ``torch.optim.Adam`` step on this Q-Former's flat master / gradient buffers on the HIP extension
        (``mra_qformer_adam_step``): update, refresh of every device weight copy (operand dtype + transposed training copies) and, with
        ``zero_grad``, the clearing of the gradient buffer in ONE pass.  The moments live in two flat fp32 buffers created here."""
        self.enable_training()
        if getattr(self, "_exp_avg", None) is None:
            self._exp_avg = torch.zeros_like(self._master_flat)
            self._exp_avg_sq = torch.zeros_like(self._master_flat)
            self._adam_t = 0
        self._bind_master()
        self._adam_t += 1
        with torch.cuda.device(self._device):
            check(lib().mra_qformer_adam_step(self._handle, ptr(self._master_flat), ptr(self._grad_flat), ptr(self._exp_avg), ptr(self._exp_avg_sq),
                                              self._master_flat.numel() * 4, float(lr), float(betas[0]), float(betas[1]), float(eps),
                                              float(weight_decay), int(self._adam_t), int(bool(zero_grad)), current_stream()), "mra_qformer_adam_step")
        # the pass refreshed the device copies itself: nothing is stale (the version counters were not bumped either)
        self._param_version = sum(p._version for p in self.bert.parameters())
        self._dirty = False
        self._grads_zeroed = bool(zero_grad)

    def _enc_grad(self, enc, N, L, Kv, prompts: int, workspace) -> torch.Tensor:
        """``mra_qformer_backward_enc`` on the tape the backward just walked: the gradient with respect to ``enc``, in its dtype."""
        d_enc = torch.empty(N, Kv, self.cfg.enc_width, dtype=torch.float32, device=enc.device)
        with torch.cuda.device(self._device):
            check(lib().mra_qformer_backward_enc(self._handle, N, prompts, L, Kv, ptr(workspace), workspace.numel(), ptr(d_enc), current_stream()),
                  "mra_qformer_backward_enc")
        return d_enc.to(enc.dtype)

    def _run_backward(self, input_ids, attention_mask, enc, N, L, Kv, d_q, d_c, prompts: int, workspace) -> None:
        # optimizer.zero_grad(set_to_none=True) drops the views: start from a clean buffer in that case
        probe = self.bert.embeddings.LayerNorm.weight
        fp = getattr(self, "_flat_param", None)
        if (fp is not None and fp.grad is None) or (fp is None and probe.grad is None):
            self._grad_flat.zero_()
        if fp is not None:
            fp.grad = self._grad_flat
        with torch.cuda.device(self._device):      # N encoder items x `prompts` chain items over the node's tape
            check(lib().mra_qformer_backward_multi(self._handle, ptr(input_ids), ptr(attention_mask), ptr(enc), N, prompts, L, Kv, ptr(d_q),
                                                   ptr(d_c), ptr(self._grad_flat), ptr(workspace), workspace.numel(), current_stream()),
                  "mra_qformer_backward_multi")
        self._bind_grads()
        binder = getattr(self, "_extra_grad_binder", None)
        if binder is not None:
            binder()
        # A backward is followed by an optimizer step sooner or later, and fused optimizers (torch._fused_adam_)
        # update parameters WITHOUT bumping their version counters: presume the device copies stale from here on.
        self._dirty = True


# --------------------------------------------------------------------------------------------------
# training (BASELINE config 5): forward with an activation tape + HIP backward behind torch.autograd
# --------------------------------------------------------------------------------------------------
class _QFormerTrainFn(torch.autograd.Function):
    """Autograd node around ``mra_qformer_forward_multi_train`` / ``mra_qformer_backward_multi`` (``prompts == 1``: the single-prompt
    step, launch for launch).  The parameters live inside the handle, so the node takes an anchor tensor that requires grad; its backward
    runs the HIP backward, which ADDS into the owner's flat f32 gradient buffer (``QFormer.grad_of``).  The node owns its tape: it takes
    the owner's spare buffer if that is large enough (a fresh one otherwise), holds it in ``ctx.ws`` until its backward and
    ``_enc_grad`` have run, and hands it back -- a forward / backward loop reuses one buffer, overlapping nodes never share one."""

    @staticmethod
    def forward(ctx, anchor, owner, input_ids, attention_mask, enc, prompts, want_cls):
        cfg = owner.cfg
        N, Kv = int(enc.shape[0]), int(enc.shape[1])
        L = 0 if input_ids is None else int(input_ids.shape[1])
        dev = enc.device
        out_q = torch.empty(N * prompts, cfg.n_query, cfg.hidden, dtype=torch.float32, device=dev)
        out_c = torch.empty(N * prompts, cfg.hidden, dtype=torch.float32, device=dev) if want_cls else None
        with torch.cuda.device(dev):
            nbytes = int(lib().mra_qformer_multi_train_workspace_bytes(owner._handle, N, prompts, L, Kv))
            ws, owner._train_ws = owner._train_ws, None
            if ws is None or ws.numel() < nbytes:
                ws = None
                ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
            check(lib().mra_qformer_forward_multi_train(owner._handle, ptr(input_ids), ptr(attention_mask), ptr(enc), N, prompts, L, Kv, ptr(out_q),
                                                        ptr(out_c), ptr(ws), ws.numel(), current_stream()),
                  "mra_qformer_forward_multi_train")
        ctx.owner, ctx.shape, ctx.ws = owner, (N, prompts, L, Kv), ws
        ctx.save_for_backward(input_ids, attention_mask, enc)
        ctx.want_cls = want_cls
        return (out_q, out_c) if want_cls else (out_q, torch.empty(0, device=dev))

    @staticmethod
    def backward(ctx, d_q, d_c):
        owner = ctx.owner
        input_ids, attention_mask, enc = ctx.saved_tensors
        N, P, L, Kv = ctx.shape
        d_q = None if d_q is None else d_q.to(torch.float32).contiguous()
        d_c = d_c.to(torch.float32).contiguous() if (ctx.want_cls and d_c is not None) else None
        owner._run_backward(input_ids, attention_mask, enc, N, L, Kv, d_q, d_c, P, ctx.ws)
        d_enc = owner._enc_grad(enc, N, L, Kv, P, ctx.ws) if ctx.needs_input_grad[4] else None      # reads the tape the backward just walked
        if owner._train_ws is None or owner._train_ws.numel() < ctx.ws.numel():
            owner._train_ws = ctx.ws
        ctx.ws = None
        return torch.zeros_like(owner._anchor), None, None, None, d_enc, None, None


class _ModalityLNTrainFn(torch.autograd.Function):
    """Autograd node around ``mra_modality_ln`` / ``mra_modality_ln_backward`` (``QFormer.modality_ln_train``).  The LayerNorm's
    parameters are read from the handle (the caller pushed them); ``weight`` / ``bias`` are inputs so that autograd hands them their
    gradients."""

    @staticmethod
    def forward(ctx, x, weight, bias, owner):
        x = x.contiguous()
        ctx.owner = owner
        ctx.save_for_backward(x)
        return owner.modality_ln(x)

    @staticmethod
    def backward(ctx, d_out):
        owner = ctx.owner
        (x,) = ctx.saved_tensors
        need_x, need_g, need_b = ctx.needs_input_grad[:3]
        if not (need_x or need_g or need_b):
            return None, None, None, None
        d32 = d_out.to(torch.float32).contiguous()
        if d32.data_ptr() == d_out.data_ptr():
            d32 = d32.clone()        # d_x is written in place: never over a tensor autograd still owns
        d_x, d_g, d_b = owner._ln_backward(x, d32, need_x, need_g, need_b)
        # fused optimizers update the LayerNorm without bumping its version counter: the holder of the parameters pushes them again
        hook = getattr(owner, "_ln_grad_hook", None)
        if hook is not None and (need_g or need_b):
            hook()
        return (d_x.to(x.dtype) if need_x else None), d_g, d_b, None


class _LlmProjTrainFn(torch.autograd.Function):
    """Autograd node around ``mra_llm_proj`` / ``mra_llm_proj_backward`` (``QFormer.llm_proj_train``).  The projection's parameters are
    read from the handle (the caller pushed them); ``weight`` / ``bias`` are inputs so that autograd hands them their gradients."""

    @staticmethod
    def forward(ctx, z, weight, bias, owner, out_dtype, grad_scale):
        z2 = z.reshape(-1, owner.cfg.hidden).to(torch.float32).contiguous()
        ctx.owner, ctx.z_shape, ctx.z_dtype, ctx.grad_scale = owner, z.shape, z.dtype, grad_scale
        ctx.save_for_backward(z2)
        return owner.llm_proj(z, out_dtype)

    @staticmethod
    def backward(ctx, d_out):
        owner = ctx.owner
        (z2,) = ctx.saved_tensors
        need_z, need_w, need_b = ctx.needs_input_grad[:3]
        if not (need_z or need_w or need_b):
            return None, None, None, None, None, None
        d2 = d_out.reshape(-1, owner.cfg.llm_hidden)
        if ctx.grad_scale != 1.0:
            d2 = d2.to(torch.float32) / ctx.grad_scale
        elif d2.dtype != owner.cfg.op_dtype:
            d2 = d2.to(torch.float32)
        d_z, d_w, d_b = owner._proj_backward(z2, d2.contiguous(), need_z, need_w, need_b)
        # fused optimizers update the projection without bumping its version counter: the holder of the parameters pushes them again
        hook = getattr(owner, "_proj_grad_hook", None)
        if hook is not None and (need_w or need_b):
            hook()
        return (d_z.reshape(ctx.z_shape).to(ctx.z_dtype) if need_z else None), d_w, d_b, None, None, None
