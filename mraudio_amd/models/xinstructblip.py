"""``XInstructBLIP`` with the reference's Python surface, its encode/fuse hot path on MI355X kernels.

Mirrors ``models/xinstructblip.py`` of the reference (class at ``:51``):

* ``XInstructBLIP(model_path, audio_path)``; attributes ``{m}_encoder``, ``{m}_ln``, ``{m}_Qformer``,
  ``{m}_query_tokens``, ``{m}_llm_proj`` with the checkpoint key names the reference's loader routes
  (``:769-816``); ``.generate(samples) -> list[str]`` (``:222``), ``.forward(samples) -> {"loss"}``
  (``:399``), ``.load_state_dict`` returning ``_IncompatibleKeys``, ``.get_optimizer_params``.
* ``samples`` schema as produced by ``utils/mr_dataset.py`` + ``collate_fn``:
  ``video [B,3,T,224,224]``, ``audio [B,T,F,128]``, ``text_input``, ``timestamps``, ``duration``.

What differs, on purpose: the reference hands the projected query embeddings to an
8-bit Vicuna-7B and parses generated text; here ``generate`` scores clips with the cosine scorer and
formats the span as the same ``"[[start, end]]"`` string, so ``evaluate.py``-shaped callers
(``moment_str_to_list(post_process(out))``, ``evaluate.py:48``) run unchanged.  The ViT-g / BEATs
encoders (row A1) are pluggable modules (``audio_encoder="beats"`` builds the HIP BEATs encoder, ``models/beats.py``); pre-computed encoder outputs can be passed
as ``samples["video_embeds"] [B,T,Kv,1408]`` / ``samples["audio_embeds"] [B,T,Kv,768]``.  With ``audio_processor=`` a device
``BeatsAudioProcessor``, audio may also enter as raw 16 kHz waveforms, ``samples["audio_wave"]`` (a list of B tensors or ``[B, samples]``,
``samples["audio"]`` absent): the filterbank is computed on the GPU (``csrc/fbank.hip``) and T is the processor's ``n_frames``.
``samples["audio_wave_rate"]`` (an int, or a list of B ints; the processor built with ``resample="sinc"``) gives the waveforms' own
sample rates: each clip goes up as decoded, ``[samples]`` or ``[channels, samples]``, and is band-limited to 16 kHz mono on the GPU
(``csrc/resample.hip``) in front of the filterbank.  Without the key nothing changes.  Likewise with ``video_processor=`` a device Alpro
video processor: ``samples["video_raw"]`` (decoded uint8 frames ``[B, T, H, W, 3]`` or a list of B clips, ``samples["video"]`` absent) with
the optional clip-wide ``samples["video_box"]`` / ``samples["video_flip"]`` is cropped, resized, flipped and normalised on the GPU
(``csrc/video_pre.hip``) into the f16 pixels the video encoder reads; T is the processor's ``n_frms``.

All arithmetic between the encoder output and the span runs in ``libmra_hip.so``: modality
LayerNorm + reorder (``:265,281-285``), Q-Former (``:286-293``), slice + llm_proj (``:303-306``),
scorer.  No CPU fallback exists.
"""
from __future__ import annotations

import contextlib
import logging
import re
import zlib
from typing import Dict, List, Optional, Sequence

import torch
import torch.nn as nn
from torch.nn.modules.module import _IncompatibleKeys

from .. import parallel, scorer
from .._lib import MraError
from ..qformer import QFormer, QFormerConfig, draw_seeded
from ..utils.mr_dataset import bpt_index, pad_queries


class HashTokenizer:
    """Offline stand-in for ``BertTokenizer("bert-base-uncased")`` (reference ``:609-612``), whose
    vocabulary file is a network download.  Lower-cased words and punctuation map to stable ids in
    [1000, 30521] by CRC32; [CLS]=101, [SEP]=102, [PAD]=0; same call signature and outputs
    (``input_ids``, ``attention_mask``, right padding to the longest, left truncation).
    Token ids are synthetic: use the real tokenizer with real checkpoints."""

    cls_id, sep_id, pad_id = 101, 102, 0

    def __init__(self, truncation_side: str = "left"):
        self.truncation_side = truncation_side

    def __len__(self):
        return 30523

    def _encode(self, text: str, max_length: int) -> List[int]:
        words = re.findall(r"[a-z0-9]+|[^\sa-z0-9]", text.lower())
        ids = [1000 + zlib.crc32(w.encode()) % 29522 for w in words]
        room = max_length - 2
        if len(ids) > room:
            ids = ids[-room:] if self.truncation_side == "left" else ids[:room]
        return [self.cls_id] + ids + [self.sep_id]

    def __call__(self, text, padding="longest", truncation=True, max_length=128, return_tensors="pt", **unused):
        texts = [text] if isinstance(text, str) else list(text)
        enc = [self._encode(t, max_length) for t in texts]
        width = max(len(e) for e in enc)
        ids = torch.full((len(enc), width), self.pad_id, dtype=torch.long)
        att = torch.zeros((len(enc), width), dtype=torch.long)
        for i, e in enumerate(enc):
            ids[i, : len(e)] = torch.tensor(e)
            att[i, : len(e)] = 1
        return _Encoding(ids, att)


class _Encoding:
    def __init__(self, input_ids, attention_mask):
        self.input_ids, self.attention_mask = input_ids, attention_mask

    def to(self, device):
        return _Encoding(self.input_ids.to(device), self.attention_mask.to(device))


class LayerNorm(nn.Module):
    """``{modality}_ln`` (reference ``:822-828``): fp32 LayerNorm, eps 1e-5, result in the input dtype.
    Parameter container; called directly it runs the HIP modality-LN kernel and returns the operand
    dtype tensor the Q-Former consumes."""

    def __init__(self, num_features: int):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(num_features), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(num_features), requires_grad=False)
        object.__setattr__(self, "_qformer_ref", None)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        qf = self._qformer_ref()
        shape = x.shape
        return qf.modality_ln(x.reshape(-1, shape[-2], shape[-1])).reshape(shape)


class _Proj(nn.Module):
    def __init__(self, in_f: int, out_f: int):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_f, in_f), requires_grad=False)
        self.bias = nn.Parameter(torch.empty(out_f), requires_grad=False)
        object.__setattr__(self, "_qformer_ref", None)

    def forward(self, z: torch.Tensor) -> torch.Tensor:
        return self._qformer_ref().llm_proj(z)


class _ScaleGrad(torch.autograd.Function):
    """Identity whose gradient is multiplied by ``scale`` (``XInstructBLIP.loss_scale``: the value of the LM loss stays the loss)."""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.scale, None


ENC_WIDTH = {"video": 1408, "audio": 768}  # EVA ViT-g / BEATs num_features (reference :123)


# ---- host steps that read no model state: every path through XInstructBLIP shares them ------------------------
def _encode_chunked(encoder, frames: torch.Tensor, chunk: int) -> torch.Tensor:
    """``encoder`` over ``frames`` [n, ...] in pieces of ``chunk`` frames under ``no_grad``: the concatenation of its outputs."""
    outs = []
    with torch.no_grad():
        for c0 in range(0, int(frames.shape[0]), max(1, int(chunk))):
            outs.append(encoder(frames[c0: c0 + chunk]))
    return outs[0] if len(outs) == 1 else torch.cat(outs)


def _timestamps(samples, bs: int, num: int) -> List[list]:
    """Per video the timestamps of its ``num`` positions as a list: ``samples["timestamps"]`` (tensors converted), else ``range(num)``."""
    ts = samples.get("timestamps")
    if ts is None or len(ts) == 0:      # (the training targets have always taken an empty list as absent)
        ts = [list(range(num))] * bs
    return [t.tolist() if torch.is_tensor(t) else list(t) for t in ts]


def _is_grouped(samples) -> bool:
    """One record per video with the LIST of its queries (``collate_grouped``), against one prompt string per sample."""
    ti = samples.get("text_input")
    return ti is not None and len(ti) > 0 and isinstance(ti[0], (list, tuple))


def _membership_targets(parse,windows: Sequence[str], stamps: Sequence[float], rows: torch.Tensor) -> torch.Tensor:
    """Clip-membership targets, written into the zeroed ``rows`` [len(windows), len(stamps)] and returned: row ``p`` becomes 1 where a timestamp
    lies inside ANY of the windows that ``parse`` (``XInstructBLIP.parse_windows``) reads from ``windows[p]`` (union over windows, float
    seconds honoured)."""
    t = torch.as_tensor(stamps, dtype=torch.float32, device=rows.device)
    for p, txt in enumerate(windows):
        for s0, e0 in parse(txt):
            rows[p] = torch.maximum(rows[p], ((t >= s0) & (t <= e0)).float())
    return rows


def _prompt_rows(ids: torch.Tensor, tmask: torch.Tensor, n_query: int, num: Optional[int] = None, prompts: int = 1, tile: bool = False):
    """The Q-Former chain's ``(input_ids, attention_mask)`` from tokenised prompts ``ids`` / ``tmask`` [B * prompts, L] (row ``b * prompts + p``):
    one row per (video, position, prompt), the mask with the ``n_query`` query-token ones in front.  ``tile`` is the reference's
    ``ids.repeat(num, 1)`` (``:287-288``): row k carries prompt ``k % B``.  Otherwise row ``(b * num + t) * prompts + p`` carries prompt ``p`` of
    video ``b`` -- with one prompt per video, row k carries the prompt of its own sample ``k // num``.  ``num=None``: the rows as given."""
    if num is not None:
        ids, tmask = _expand_rows(ids, num, prompts, tile), _expand_rows(tmask, num, prompts, tile)
    ones = torch.ones(tmask.shape[0], n_query, dtype=torch.long, device=tmask.device)
    return ids, torch.cat([ones, tmask], dim=1)


def _expand_rows(x: torch.Tensor, num: int, prompts: int = 1, tile: bool = False) -> torch.Tensor:
    """One of ``ids`` / ``tmask`` in ``_prompt_rows``' row order, ``[B * num * prompts, L]``."""
    if tile:
        return x.repeat(num, 1)
    bs, L = int(x.shape[0]) // prompts, int(x.shape[1])
    return x.view(bs, 1, prompts, L).expand(bs, num, prompts, L).reshape(bs * num * prompts, L)


def _train_logit(z: torch.Tensor, cls: torch.Tensor) -> torch.Tensor:
    """The scorer logit of the training paths as torch ops: per row ``max_q cos(z[q], cls)``."""
    return nn.functional.cosine_similarity(z, cls[:, None, :], dim=-1, eps=1e-8).max(dim=1).values


def _weighted_fuse(per_mod: Sequence[torch.Tensor], weights: Optional[Sequence[float]]) -> torch.Tensor:
    """The weighted sum of the per-modality training logits (default: their mean)."""
    w = weights or [1.0 / len(per_mod)] * len(per_mod)
    return sum(x * wt for x, wt in zip(per_mod, w))


def _store_scores(out: Dict[str, object], m: str, z: torch.Tensor, cls: torch.Tensor):
    """``cosine_scores`` of one modality's rows into ``out["z" / "cls" / "sim" / "logit"][m]``; returns ``(sim, logit)``."""
    sim, logit = scorer.cosine_scores(z, cls)
    out["z"][m], out["cls"][m], out["sim"][m], out["logit"][m] = z, cls, sim, logit
    return sim, logit


def _span_texts(spans: torch.Tensor, ts: Sequence[list]) -> List[str]:
    """One ``"[[start, end]]"`` string (seconds) per row of ``spans`` [n, 2]; ``ts[i]`` the timestamps row ``i`` indexes."""
    return [o.strip() for o in scorer.spans_to_text(spans.cpu().tolist(), ts)]


def _window_texts(win: torch.Tensor, sc: torch.Tensor, cnt: torch.Tensor, ts: Sequence[list]):
    """``(texts, records)`` of ranked windows ``win`` [n, k, 2] / ``sc`` [n, k] / ``cnt`` [n]; ``ts[i]`` the timestamps row ``i`` indexes."""
    win, sc, cnt = win.cpu(), sc.cpu(), cnt.cpu()
    return scorer.windows_to_text(win, cnt, ts), scorer.windows_to_records(win, sc, cnt, ts)


LM_DECODES, LM_PREFILLS = ("stock", "hip", "hip_step"), ("stock", "hip")       # XInstructBLIP.lm_decode / .lm_prefill; the CLIs' choices
LM_ATTENTIONS = ("stock", "hip")                                                # XInstructBLIP.lm_attention


def check_lm_options(lm_decode: str, lm_prefill: str = "stock", unknown_decode=ValueError) -> None:
    """The one rule for the pair: ``lm_decode`` in ``LM_DECODES`` (``unknown_decode`` otherwise), ``lm_prefill`` in ``LM_PREFILLS``, and
    "hip" needs ``lm_decode`` "hip" or "hip_step" (ValueError otherwise)."""
    if lm_decode not in LM_DECODES:
        raise unknown_decode(f"lm_decode must be 'stock', 'hip' or 'hip_step', got {lm_decode!r}")
    if lm_prefill not in LM_PREFILLS:
        raise ValueError(f"lm_prefill must be 'stock' or 'hip', got {lm_prefill!r}")
    if lm_prefill == "hip" and lm_decode == "stock":
        raise ValueError(f"lm_prefill='hip' needs lm_decode 'hip' or 'hip_step' (the stock decode is the reference's call, untouched), got lm_decode={lm_decode!r}")


def check_lm_prefill(lm_prefill: str, lm_decode: str) -> None:
    """``check_lm_options`` under its earlier name and argument order."""
    check_lm_options(lm_decode, lm_prefill)


def _lm_ce_call(self, embeds, mask, targets):
    """``XInstructBLIP._lm_ce`` under the attention implementation the LM has at this moment."""
    if self.lm_loss == "stock":
        return self.llm_model(inputs_embeds=embeds, attention_mask=mask, return_dict=True, labels=targets).loss
    if self.lm_loss not in ("rows", "fused"):
        raise MraError(f"lm_loss must be 'stock', 'rows' or 'fused', got {self.lm_loss!r}")
    from .lm_head import lm_head_ce

    llm = self.llm_model
    prefix = getattr(llm, "base_model_prefix", "")
    dec = llm.get_decoder() if hasattr(llm, "get_decoder") else (getattr(llm, prefix, None) if prefix else None)
    if dec is None or dec is llm:
        raise MraError(f"lm_loss {self.lm_loss!r} needs an LM that exposes its decoder (get_decoder() or its base_model_prefix attribute)")
    head = llm.get_output_embeddings() if hasattr(llm, "get_output_embeddings") else None
    if head is None or getattr(head, "weight", None) is None:
        raise MraError(f"lm_loss {self.lm_loss!r} needs an LM with an output embedding (get_output_embeddings())")
    if getattr(head, "bias", None) is not None:
        raise MraError(f"lm_loss {self.lm_loss!r}: the LM's output embedding has a bias, which the row-wise head does not take")
    hidden = dec(inputs_embeds=embeds, attention_mask=mask, return_dict=True).last_hidden_state
    return lm_head_ce(hidden, head.weight, targets, hip=False if self.lm_loss == "rows" else None)


class XInstructBLIP(nn.Module):
    # what forward() trains on: "score" (the build-defined scorer loss), "llm" (the attached LM's cross-entropy on the answer tokens,
    # reference :399-606) or "both" (bce + lm_weight * lm over ONE Q-Former forward per modality).  loss_scale: the LM term's
    # gradient is multiplied by it on its way into the LM and divided out again in the projection's backward (see forward_llm)
    objective, lm_weight, loss_scale = "score", 1.0, 1.0
    lora = False                                 # LoRA adapters inside the attached LM (enable_lora): the reference's own trainable set
    # how the LM loss is computed (_lm_ce): "stock" = the LM's own forward with labels (lm_head over every position), "rows" = the LM's decoder,
    # then lm_head + cross-entropy on the labelled rows only as torch ops, "fused" = the same on the HIP entries (models/lm_head.py)
    lm_loss = "stock"
    # how the prompt in front of the LM is put together: "cat" = PromptAssembler.assemble_* (torch.cat of its pieces), "plan" = a PromptPlan
    # executed as one row gather (models/llm_prompt.py assemble_plan; mra_gather_rows).  Grouped batches always take the plan
    prompt_assembly = "cat"
    # the LM objective ("llm" / "both") on grouped batches (several queries per video: forward_multi's pass + the plan).  Off: such a batch
    # is refused with MraError, as it always was
    grouped_lm = False
    # how generate_llm / generate_multi_llm decode (_llm_decode): "stock" = llm_model.generate as it comes (a growing cache, SDPA), "hip" = the
    # same greedy generate over a static cache with the one-token attention on mra_decode_attention (models/lm_decode.py), "hip_step" = the
    # prefill through the LM's own forward, then one mra_lm_step per token (models/lm_step.py)
    lm_decode = "stock"
    # the prefill in front of that decode: "stock" = the LM's forward as it is configured (SDPA under the [S, S] bool mask), "hip" = the same
    # forward with its attention on mra_prefill_attention under the key mask alone (models/lm_decode.py).  "hip" needs lm_decode "hip" or
    # "hip_step": the stock decode is the reference's call and stays untouched
    lm_prefill = "stock"
    # the LM's attention in the training pass (_lm_ce): "stock" = the LM's forward as it is configured (SDPA under the [S, S] bool mask, forward
    # and backward), "hip" = the same forward inside lm_attention.hip_train: the causal attention as one autograd node on mra_prefill_attention
    # and mra_prefill_attention_backward under the key mask alone (models/lm_attention.py).  Independent of lm_decode / lm_prefill
    lm_attention = "stock"

    def __init__(self, model_path: Optional[str] = None, audio_path: Optional[str] = None, *,
                 modalities: Optional[Sequence[str]] = None, video_encoder: Optional[nn.Module] = None,
                 audio_encoder=None, tokenizer=None, seed: Optional[int] = 0,
                 perturb: bool = False, op_dtype: torch.dtype = torch.float16, device=None,
                 compat_repeat: bool = True, score_alpha: float = 0.5, fuse_weights: Optional[Sequence[float]] = None,
                 process_group=None, qformer_overrides: Optional[dict] = None, overlap_modalities: bool = True,
                 llm_hidden_size: int = 4096, checkpoint: Optional[str] = None, checkpoint_strict: bool = True,
                 cross_precision: str = "op", audio_processor=None, top_k: int = 1, nms_thd: float = 0.25, max_window: int = 0,
                 video_processor=None, lm_loss: str = "stock", prompt_assembly: str = "cat",
                 grouped_lm: bool = False, lm_decode: str = "stock", lm_prefill: str = "stock", lm_attention: str = "stock"):
        super().__init__()
        check_lm_options(lm_decode, lm_prefill)
        self.lm_decode, self.lm_prefill = lm_decode, lm_prefill
        if lm_attention not in LM_ATTENTIONS:
            raise ValueError(f"lm_attention must be 'stock' or 'hip', got {lm_attention!r}")
        self.lm_attention = lm_attention
        if lm_loss not in ("stock", "rows", "fused"):
            raise ValueError(f"lm_loss must be 'stock', 'rows' or 'fused', got {lm_loss!r}")
        self.lm_loss = lm_loss
        if prompt_assembly not in ("cat", "plan"):
            raise ValueError(f"prompt_assembly must be 'cat' or 'plan', got {prompt_assembly!r}")
        self.prompt_assembly = prompt_assembly
        self.grouped_lm = bool(grouped_lm)
        self.model_path, self.audio_path = model_path, audio_path
        self.modalities = list(modalities) if modalities is not None else ["audio", "video"]  # reference :71
        self.max_txt_len = 128           # reference :75
        self.max_output_txt_len = 64
        self.num_query_token = 32        # reference :120
        self.compat_repeat = compat_repeat
        self.score_alpha = score_alpha
        # ranked proposals (the scorer's windows kernel, _score_tail): with top_k > 1 fuse_score also returns the top_k windows under temporal NMS
        # (threshold nms_thd, window length capped at max_window clips, 0 = none); 1 = the single span only, no extra launch
        self.top_k, self.nms_thd, self.max_window = int(top_k), float(nms_thd), int(max_window)
        self.fuse_weights = fuse_weights
        self.process_group = process_group
        # True: the clips of one batch are sharded over the ranks (inference, every rank is given the same
        # samples).  False: ranks hold different samples (data-parallel training, utils/trainer.py) and only
        # gradients are exchanged.
        self.clip_parallel = True
        self.overlap_modalities = overlap_modalities
        self.pair_forward = False        # see fuse_score: two modalities of equal Q-Former shape as ONE launch sequence (mra_qformer_forward_pair); measured slower, opt-in
        self.kv_first = True             # see fuse_score: light modalities wait for the heavy K/V projection
        self.prioritize_heavy = True     # see fuse_score
        self.encode_chunk = 64           # frames per encoder call of the batched [B*T] encode (row A1)
        self.roofline_events = None      # bench instrumentation: {modality: (start, stop) events}
        self._streams: Dict[str, torch.cuda.Stream] = {}
        self._device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.tokenizer = tokenizer if tokenizer is not None else self.init_tokenizer(truncation_side="left")
        self.video_encoder = video_encoder
        if isinstance(audio_encoder, str):   # "beats": the reference's init_audio_encoder (:670-676), BeatsEncoder(audio_path) on the HIP kernels
            if audio_encoder != "beats":
                raise ValueError(f"audio_encoder: an nn.Module, None or 'beats', got {audio_encoder!r}")
            from .beats import BeatsEncoder
            audio_encoder = BeatsEncoder(checkpoint_path=audio_path, backend="hip", device=self._device)
        self.audio_encoder = audio_encoder
        # a device BeatsAudioProcessor (processors/audio_processors.py): samples["audio_wave"] becomes the step's filterbank on the GPU
        # (mra_fbank_forward) and goes to audio_encoder without leaving it; its n_frames is T
        self.audio_processor = audio_processor
        # a device Alpro video processor (processors/alpro_processors.py): samples["video_raw"], the decoded uint8 frames, become the
        # encoder's normalised f16 pixels on the GPU (mra_video_frames_forward: crop, resize, flip, normalise); its n_frms is T
        self.video_processor = video_processor
        self.llm_hidden_size = llm_hidden_size   # Vicuna-7B: 4096 (reference :167)
        self.llm_model = None                    # stock causal LM, attached by attach_llm (row N2)
        self.llm_tokenizer = None
        self.prompt_assembler = None
        gen = torch.Generator().manual_seed(seed) if seed is not None else None
        # synthetic init draws modalities in sorted order so the tensors do not depend on list order
        for m in sorted(self.modalities):
            cfg = QFormerConfig(enc_width=ENC_WIDTH[m], op_dtype=op_dtype, llm_hidden=self.llm_hidden_size,
                                **(qformer_overrides or {}))
            qf, qt = self.init_Qformer(self.num_query_token, ENC_WIDTH[m], cfg=cfg, device=self._device)
            if cross_precision != "op":   # "split" / "auto": QFormer.set_cross_precision (inference forwards only)
                qf.set_cross_precision(cross_precision)
            setattr(self, f"{m}_Qformer", qf)
            setattr(self, f"{m}_query_tokens", qt)
            ln = self.init_ln(ENC_WIDTH[m])
            proj = self.init_vicuna_projection(cfg.hidden, self.llm_hidden_size)
            setattr(self, f"{m}_ln", ln)
            setattr(self, f"{m}_llm_proj", proj)
            object.__setattr__(ln, "_qformer_ref", _ref(qf))
            object.__setattr__(proj, "_qformer_ref", _ref(qf))
            if gen is not None:
                mg = torch.Generator().manual_seed(int(seed) + (0 if m == "video" else 1))
                qf.init_seeded_(perturb=perturb, gen=mg)
                qt.data.copy_(draw_seeded(mg, (1, cfg.n_query, cfg.hidden), "w", perturb))
                ln.weight.data.copy_(draw_seeded(mg, (cfg.enc_width,), "g", perturb))
                ln.bias.data.copy_(draw_seeded(mg, (cfg.enc_width,), "z", perturb))
                proj.weight.data.copy_(draw_seeded(mg, (self.llm_hidden_size, cfg.hidden), "w", perturb))
                proj.bias.data.copy_(draw_seeded(mg, (self.llm_hidden_size,), "b", perturb))
        self.to(self._device)
        self._extras_dirty = True
        # Where the Q-Former / LN / projection weights come from.  The reference downloads them in its constructor
        # (``:79-194``; ``model_path`` there is the Vicuna directory, ``audio_path`` the BEATs checkpoint); offline they
        # come from ``checkpoint`` (a state dict with the reference's key names) or stay the seeded synthetic init.
        self.weights_source = f"synthetic (seed {seed})"
        if checkpoint is not None:   # strict like the reference's load_checkpoint; checkpoint_strict=False = its load_from_pretrained (a trainer checkpoint holds trainable parameters only)
            self.load_checkpoint(checkpoint) if checkpoint_strict else self.load_from_pretrained(checkpoint)
        elif model_path is not None or audio_path is not None:
            logging.warning("XInstructBLIP(model_path=%r, audio_path=%r): no checkpoint was given, the Q-Former / LayerNorm / "
                            "projection weights are the SYNTHETIC seeded init -- predictions are not meaningful.  Pass "
                            "checkpoint=<state dict .pth> (evaluate.py / finetune.py: --checkpoint).", model_path, audio_path)

    # ---- construction helpers with the reference's names (:609-735) --------------------------------
    @classmethod
    def init_tokenizer(cls, truncation_side="right"):
        try:  # the real vocabulary when it is on disk; never a download
            from transformers import BertTokenizer
            tok = BertTokenizer.from_pretrained("bert-base-uncased", truncation_side=truncation_side, local_files_only=True)
            tok.add_special_tokens({"bos_token": "[DEC]"})
            return tok
        except Exception:
            logging.info("bert-base-uncased vocabulary not on disk: using the offline HashTokenizer")
            return HashTokenizer(truncation_side=truncation_side)

    @classmethod
    def init_Qformer(cls, num_query_token, modality_width, cross_attention_freq=2, cfg: Optional[QFormerConfig] = None,
                     device=None):
        cfg = cfg or QFormerConfig(enc_width=modality_width, cross_freq=cross_attention_freq, n_query=num_query_token)
        qformer = QFormer(cfg, device=device)
        query_tokens = nn.Parameter(torch.zeros(1, num_query_token, cfg.hidden), requires_grad=False)
        return qformer, query_tokens

    @classmethod
    def init_ln(cls, num_features, load_ln_path=False, load_ln_type=""):
        return LayerNorm(num_features)

    @classmethod
    def init_vicuna_projection(cls, input_size, output_size, load_projection_path=False, load_projection_type="", projection_key=None):
        return _Proj(input_size, output_size)

    @property
    def device(self):
        return self._device

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._extras_dirty = True
        return out

    # ---- checkpoints (reference :737-816) --------------------------------------------------------------
    def load_state_dict(self, state_dict, strict=True, assign=False):
        """Routes ``{m}_Qformer.*``, ``{m}_query_tokens``, ``{m}_ln.*``, ``{m}_llm_proj.*`` as the
        reference does (``:769-816``); encoder keys are ignored.  ``llm_model.*`` keys are ignored too (no LLM on this path) unless
        ``enable_lora()`` was called: then, as in the reference (``:807-813``), they go into the LM's adapters (``load_lora_state_dict``);
        adapter keys the file lacks are listed as missing ``llm_model.*`` keys but, as there (``:815``), never make ``strict`` raise.
        A file whose keys are ALL ``llm_model.*`` -- what the reference's trainer writes, and this one's with frozen Q-Formers -- is an
        adapter file: with LoRA on it says nothing about the Q-Former side, which keeps its weights and is neither reported nor raised on."""
        missing, unexpected = [], []
        for m in self.modalities:
            sub = {".".join(k.split(".")[1:]): v for k, v in state_dict.items() if k.split(".")[0] == f"{m}_Qformer"}
            msg = getattr(self, f"{m}_Qformer").load_state_dict(sub, strict=False)
            missing += [f"{m}_Qformer.{k}" for k in msg.missing_keys]
            unexpected += [f"{m}_Qformer.{k}" for k in msg.unexpected_keys]
            if f"{m}_query_tokens" not in state_dict:
                missing.append(f"{m}_query_tokens")
            else:
                getattr(self, f"{m}_query_tokens").data.copy_(state_dict[f"{m}_query_tokens"])
            for part in ("ln", "llm_proj"):
                sub = {".".join(k.split(".")[1:]): v for k, v in state_dict.items() if k.split(".")[0] == f"{m}_{part}"}
                msg = nn.Module.load_state_dict(getattr(self, f"{m}_{part}"), sub, strict=False)
                missing += [f"{m}_{part}.{k}" for k in msg.missing_keys]
                unexpected += [f"{m}_{part}.{k}" for k in msg.unexpected_keys]
        known = tuple(f"{m}_" for m in self.modalities)
        unexpected += [k for k in state_dict if not k.startswith(known) and k.split(".")[0] != "llm_model"
                       and "encoder" not in k.split(".")[0]]
        self._extras_dirty = True
        lora_missing = []
        lora_sd = {k[len("llm_model."):]: v for k, v in state_dict.items() if k.startswith("llm_model.")} if self.lora else {}
        if lora_sd:
            from .lora import load_lora_state_dict
            miss, unexp = load_lora_state_dict(self.llm_model, lora_sd)
            lora_missing = [f"llm_model.{k}" for k in miss]
            unexpected += [f"llm_model.{k}" for k in unexp]
            if all(k.startswith("llm_model.") for k in state_dict):
                missing = []
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for XInstructBLIP: missing {missing}, unexpected {unexpected}")
        return _IncompatibleKeys(missing + lora_missing, unexpected)

    def _load_file(self, filename, strict: bool):
        ckpt = torch.load(filename, map_location="cpu", weights_only=True)
        sd = ckpt["model"] if "model" in ckpt else ckpt
        mine = [k for k in sd if k.startswith(tuple(f"{m}_" for m in self.modalities))]
        if not mine and not (self.lora and any(k.startswith("llm_model.") for k in sd)):
            raise RuntimeError(f"{filename}: no key of this model's modalities {self.modalities} found")
        msg = self.load_state_dict(sd, strict=strict)
        if not mine:            # an adapter file: the Q-Former side is what it was
            self.weights_source = f"{getattr(self, 'weights_source', 'seeded init')} + LoRA adapters of {filename}"
            return msg
        self.weights_source = f"checkpoint {filename}"
        if msg.missing_keys:
            self.weights_source += f" ({len(msg.missing_keys)} parameters NOT in the file keep their previous values)"
            logging.warning("%s: %d parameters keep their previous values (first: %s)", filename, len(msg.missing_keys), msg.missing_keys[:3])
        if isinstance(self.tokenizer, HashTokenizer):
            logging.warning("checkpoint weights are used with the offline HashTokenizer: token ids do NOT match the "
                            "bert-base-uncased vocabulary the checkpoint was trained with")
        return msg

    def load_checkpoint(self, filename, strict: bool = True, **kwargs):
        """Weights-only load of a finetuned ``.pth`` holding the reference's key names (``{m}_Qformer.*``, ``{m}_query_tokens``,
        ``{m}_ln.*``, ``{m}_llm_proj.*``; optionally under ``"model"``).  STRICT, like the reference's ``load_checkpoint``
        (``:759-767``: "this should expect no mismatch in the model keys and the checkpoint keys"): a file that lacks any
        Q-Former / LayerNorm / projection parameter of this model raises instead of silently keeping the synthetic init
        (``llm_model.*`` and encoder keys are not part of this path and are ignored).  ``strict=False`` is an explicit opt-in
        (or use ``load_from_pretrained``); the number of missing parameters then shows in ``weights_source``."""
        return self._load_file(filename, strict)

    def load_from_pretrained(self, filename, **kwargs):
        """The reference's non-strict loader (``:749-757``, ``load_state_dict(strict=False)``): partial files are accepted, what is
        missing keeps its previous values and is counted in ``weights_source``."""
        return self._load_file(filename, False)

    def get_optimizer_params(self, weight_decay, lr_scale=1):
        """LAVIS ``BaseModel.get_optimizer_params`` semantics (reference ``:818-820``): parameters that
        require grad, split into decay / no-decay (ndim < 2, bias, ln, bn) groups."""
        decay, no_decay = [], []
        for n, p in self.named_parameters():
            if not p.requires_grad:
                continue
            (no_decay if p.ndim < 2 or "bias" in n or "ln" in n or "bn" in n else decay).append(p)
        return [{"params": decay, "weight_decay": weight_decay, "lr_scale": lr_scale},
                {"params": no_decay, "weight_decay": 0, "lr_scale": lr_scale}]

    def _present(self, samples, m: str) -> bool:
        """Whether ``samples`` carries modality ``m``: its encoder input, pre-computed encoder outputs, or (audio) raw waveforms."""
        return m in samples or f"{m}_embeds" in samples or (m == "audio" and "audio_wave" in samples) or (m == "video" and "video_raw" in samples)

    def _clip_world(self):
        return parallel.world(self.process_group) if self.clip_parallel else (0, 1)

    def _gather(self, rows: torch.Tensor, n_total: int) -> torch.Tensor:
        return parallel.all_gather_rows(rows, n_total, self.process_group) if self.clip_parallel else rows

    def _kv_done_event(self, modality: str) -> torch.cuda.Event:
        """The event the library records after ``modality``'s K/V projection (``mra_qformer_set_kv_done_event``)."""
        qf: QFormer = getattr(self, f"{modality}_Qformer")
        ev = getattr(qf, "_kv_done_event", None)
        if ev is None:
            from .. import _lib
            ev = torch.cuda.Event()
            with torch.cuda.device(self._device):
                ev.record()                       # torch creates the hipEvent lazily on the first record
            _lib.check(_lib.lib().mra_qformer_set_kv_done_event(qf._handle, ev.cuda_event), "set_kv_done_event")
            qf._kv_done_event = ev
        return ev

    def _side_stream(self, modality: str, high_priority: bool = False) -> torch.cuda.Stream:
        key = (modality, high_priority)
        if key not in self._streams:
            self._streams[key] = torch.cuda.Stream(device=self._device, priority=-1 if high_priority else 0)
        return self._streams[key]

    @contextlib.contextmanager
    def _modality_streams(self, fork: bool):
        """The fork / join of the per-modality side streams.  Yields ``lane``; ``with lane(m, high_priority, after) as hand:`` runs its body
        on modality ``m``'s side stream, which first waits for the caller's stream and, if given, for the event ``after``.  The tensors
        the body passes to ``hand(...)`` (``None`` entries skipped) are consumed on the caller's stream and recorded on it.  Leaving the
        outer block joins exactly the streams that were forked.  Without ``fork`` the bodies run where they are and nothing under
        ``torch.cuda`` is touched."""
        cur = torch.cuda.current_stream(self._device) if fork else None
        forked = []

        @contextlib.contextmanager
        def lane(m: str, high_priority: bool = False, after: Optional[torch.cuda.Event] = None):
            handed = []
            if not fork:
                yield handed.extend
                return
            side = self._side_stream(m, high_priority)
            forked.append(side)
            side.wait_stream(cur)
            if after is not None:
                side.wait_event(after)
            with torch.cuda.stream(side):
                yield handed.extend
            for t in handed:
                if t is not None:
                    t.record_stream(cur)

        yield lane
        for side in forked:
            cur.wait_stream(side)

    def _tokenize(self, prompts):
        """``(input_ids, attention_mask)`` of ``prompts`` on the device, one row per prompt, padded to the longest."""
        text = self.tokenizer(prompts, padding="longest", truncation=True, max_length=self.max_txt_len, return_tensors="pt")
        return text.input_ids.to(self._device), text.attention_mask.to(self._device)

    def _qformer_input(self, qf: QFormer, x: torch.Tensor, idx: Optional[torch.Tensor], items: int):
        """What ``qf`` reads at inference, as ``(enc, raw)``: the folded cross-attention reads the encoder output itself where the library
        folds the LayerNorm into it (no normalised copy, ``raw`` True), else the ``modality_ln`` output."""
        x = x.to(self._device)
        raw = x.dim() == 3 and x.shape[0] == items and qf.raw_features_ok(x, item_index=idx)
        return (x if raw else qf.modality_ln(x, item_index=idx, items=items)), raw

    def _train_norm(self, m: str, raw: torch.Tensor, idx: Optional[torch.Tensor], items: int) -> torch.Tensor:
        """What ``{m}_Qformer`` reads in training: under ``train_ln`` the LayerNorm is a node of the graph, else it runs under ``no_grad``."""
        if getattr(self, "train_ln", False):
            return self._ln_train(m, raw)
        with torch.no_grad():
            return getattr(self, f"{m}_Qformer").modality_ln(raw, item_index=idx, items=items)

    def _pack_llm(self, out: Dict[str, object], m: str, z: torch.Tensor, bs: int, num: int):
        """Reference ``:303-306``: ``{m}_llm_proj`` of the query embeddings into ``out["inputs_llm"][m]`` [B, T * 32, D] with its
        ``out["atts_llm"][m]``; returns the two tensors."""
        y = getattr(self, f"{m}_Qformer").llm_proj(z)
        y = y.reshape(bs, num, self.num_query_token, -1).view(bs, num * self.num_query_token, -1)
        atts = torch.ones(bs, num * self.num_query_token, dtype=torch.long, device=self._device)
        out.setdefault("inputs_llm", {})[m], out.setdefault("atts_llm", {})[m] = y, atts
        return y, atts

    def _score_tail(self, logits: Sequence[torch.Tensor], videos: int, num: int) -> Dict[str, object]:
        """From per-modality logits over ``videos x num`` positions to ``fused``, ``spans`` and, with ``top_k > 1``, ``windows`` /
        ``window_scores`` / ``window_counts``."""
        out: Dict[str, object] = {"fused": scorer.fuse_logits(list(logits), self.fuse_weights)}
        out["spans"] = scorer.spans_from_logits(out["fused"], videos, num, self.score_alpha)
        if self.top_k > 1:
            out["windows"], out["window_scores"], out["window_counts"] = scorer.windows_from_logits(
                out["fused"], videos, num, self.score_alpha, self.top_k, self.nms_thd, self.max_window)
        return out

    def _sync(self):
        ver = sum(getattr(self, f"{m}_{n}")._version if n == "query_tokens" else sum(p._version for p in getattr(self, f"{m}_{n}").parameters())
                  for m in self.modalities for n in ("query_tokens", "ln", "llm_proj"))
        if ver != getattr(self, "_extras_version", None):
            self._extras_version = ver
            self._extras_dirty = True
        for m in self.modalities:
            qf: QFormer = getattr(self, f"{m}_Qformer")
            qf.sync_weights()
            if self._extras_dirty:
                qf.push("query_tokens", getattr(self, f"{m}_query_tokens"))
                qf.push("ln.weight", getattr(self, f"{m}_ln").weight)
                qf.push("ln.bias", getattr(self, f"{m}_ln").bias)
                qf.push("llm_proj.weight", getattr(self, f"{m}_llm_proj").weight)
                qf.push("llm_proj.bias", getattr(self, f"{m}_llm_proj").bias)
        self._extras_dirty = False

    # ---- the hot path -------------------------------------------------------------------------------------
    def _encode(self, samples, modality: str, lo: Optional[int] = None, hi: Optional[int] = None):
        """Row A1: the encoder calls of the reference's per-position loop (``:262-275``: ``T`` sequential
        calls at batch ``B``), collapsed to ONE sample-major ``[B*T]`` batch fed to the encoder in chunks of
        ``encode_chunk`` frames.  Item ``k = r * T + i`` of the order the reference builds afterwards with
        ``cat(embeds)[indices]`` (``:281-285``) is frame ``i`` of sample ``r``, so no gather index is needed:
        the modality LayerNorm consumes the encoder output in place.  ``[lo, hi)`` restricts the work to one
        rank's contiguous block of items (clip-sharded inference): the encoder -- 100x the Q-Former's cost --
        is sharded too, not replicated.  Returns ``(raw [hi - lo, Kv, E], None, bs, num)``."""
        key = f"{modality}_embeds"
        if key in samples:  # pre-computed encoder outputs, already sample-major [B, T, Kv, E]
            e = samples[key]
            bs, num = int(e.shape[0]), int(e.shape[1])
            e = e.reshape(bs * num, e.shape[2], e.shape[3])
            if lo is not None:
                e = e[lo:hi]
            return e.to(self._device), None, bs, num
        encoder = getattr(self, f"{modality}_encoder")
        if encoder is None:
            raise MraError(f"no {modality}_encoder was given and samples has no '{key}'")
        if modality == "audio" and modality not in samples and "audio_wave" in samples:
            # raw waveforms (a list of B tensors, or [B, samples]): the filterbank of this rank's items only, f16, computed on the device
            proc = self.audio_processor
            if proc is None or getattr(proc, "device", None) is None:
                raise MraError("samples['audio_wave'] needs XInstructBLIP(audio_processor=BeatsAudioProcessor(..., device=<cuda device>))")
            waves = samples["audio_wave"]
            waves = list(waves.unbind(0)) if isinstance(waves, torch.Tensor) else list(waves)
            bs, num = len(waves), int(proc.n_frames)
            rates = samples.get("audio_wave_rate")      # the waveforms' own sample rates: resampled on the device (csrc/resample.hip)
            frames = proc.flat(waves, lo, hi, out_dtype=torch.float16, **({} if rates is None else {"rates": rates}))
            return _encode_chunked(encoder, frames, self.encode_chunk), None, bs, num
        if modality == "video" and modality not in samples and "video_raw" in samples:
            # decoded uint8 frames ([B, T, H, W, 3] or a list of B clips): this rank's frames only go up, as bytes, and one launch
            # crops, resizes, flips and normalises them into the f16 pixels the encoder reads
            proc = self.video_processor
            if proc is None or getattr(proc, "device", None) is None:
                raise MraError("samples['video_raw'] needs XInstructBLIP(video_processor=<an Alpro video processor built with device=<cuda device>>)")
            clips = samples["video_raw"]
            bs, num = len(clips), int(proc.n_frms)
            frames = proc.flat(clips, samples.get("video_box"), samples.get("video_flip"), lo, hi, out_dtype=torch.float16)
            return _encode_chunked(encoder, frames, self.encode_chunk), None, bs, num
        data = samples[modality]
        if modality == "video":      # [B, 3, T, H, W] -> sample-major frames [B*T, 3, H, W]
            bs, num = int(data.shape[0]), int(data.shape[2])
            frames = data.permute(0, 2, 1, 3, 4).reshape(bs * num, data.shape[1], data.shape[3], data.shape[4])
        else:                        # [B, T, F, 128] -> [B*T, F, 128]
            bs, num = int(data.shape[0]), int(data.shape[1])
            frames = data.reshape(bs * num, data.shape[2], data.shape[3])
        if lo is not None:
            frames = frames[lo:hi]
        return _encode_chunked(lambda chunk: encoder(chunk.to(self._device)), frames, self.encode_chunk), None, bs, num

    @torch.no_grad()
    def fuse_score(self, embeds: Dict[str, torch.Tensor], input_ids: torch.Tensor, text_mask: torch.Tensor, bs: int, num: int,
                   index: Optional[Dict[str, torch.Tensor]] = None, want_llm: bool = False, want_full: bool = False) -> Dict[str, object]:
        """Everything after the encoders and the tokenizer, on THIS rank's block of items.

        ``embeds[m]`` raw encoder outputs; the rank's items are ``embeds[m][index[m]]`` when an index is
        given, else ``embeds[m]`` itself (``[n_local, Kv, E]``).  ``input_ids`` / ``text_mask``
        ``[n_local, L]``.  The rank's block is rows ``shard_range(bs*num, rank, world)`` of the
        sample-major item order.  LN + reorder -> Q-Former -> all-gather of the query embeddings and
        [CLS] vectors over the process group -> cosine score -> fuse -> span (identical on all ranks)."""
        self._sync()
        n = bs * num
        rank, ws = self._clip_world()
        lo, hi = parallel.shard_range(n, rank, ws)
        n_local = hi - lo
        out: Dict[str, object] = {"z": {}, "cls": {}, "sim": {}, "logit": {}, "full": {}}
        ids, att = _prompt_rows(input_ids.to(self._device), text_mask.to(self._device), self.num_query_token)
        # The modality Q-Formers are independent until the fusion: each runs on its own HIP stream so
        # the short launches of one chain fill the gaps of the other (and of its K/V projection).
        live = [m for m in self.modalities if m in embeds]
        use_streams = self.overlap_modalities and len(live) > 1
        heavy_done = None
        if use_streams:
            live.sort(key=lambda m: int(embeds[m].shape[-2]) * int(embeds[m].shape[-1]), reverse=True)
        if use_streams and self.kv_first:
            # The modality with the largest K/V projection goes first and the others start when that GEMM has
            # finished: a chip-filling GEMM gains nothing from sharing CUs with a latency-bound layer chain (it
            # ran 20 % longer beside one), whereas two layer chains overlap each other almost for free.
            heavy = live[0]
            kv_flops = 2.0 * n_local * embeds[heavy].shape[-2] * embeds[heavy].shape[-1] * 9216
            if kv_flops >= 1e12:                  # ~1 ms of GEMM; below that the wait costs more than the contention
                heavy_done = self._kv_done_event(heavy)
        sharded = ws > 1
        local: Dict[str, tuple] = {}
        if self.pair_forward and len(live) == 2 and not want_full and not want_llm and self._pair_ok(live):
            # Both Q-Formers in ONE launch sequence on the caller's stream: their layer chains have identical shapes, so every chain GEMM /
            # attention core / LayerNorm takes both modalities in one launch (0.7 ms less kernel time per headline step, folded blocks free
            # of the other stream: 0.65 instead of 0.79 ms each) -- but the two-stream form hides ~0.65 ms of the light modality behind the heavy
            # one's latency-bound chain phases, and one sequence hides nothing: 6.72-6.87 vs 6.57 ms per step, reference item shape 2.65 vs
            # 2.55 ms (r03p, same session).  Opt-in.  The heavier lane first (its cross-layer-0 block carries the roofline events).
            qfs = [getattr(self, f"{m}_Qformer") for m in live]
            # (each lane as its own forward would run it: raw features where the library folds the LayerNorm into the cross-attention)
            lanes = [self._qformer_input(qf, embeds[m], None if index is None else index.get(m), n_local) for qf, m in zip(qfs, live)]
            res = QFormer.forward_pair(qfs[0], qfs[1], ids, att, lanes[0][0], lanes[1][0], want_cls=True,
                                       kv_events=(self.roofline_events or {}).get(live[0]), raw=[raw for _, raw in lanes])
            for m, (z, cls) in zip(live, res):
                if sharded:
                    local[m] = (z, cls)
                else:
                    _store_scores(out, m, z, cls)
            live = []
        with self._modality_streams(use_streams) as lane:
            for pos, m in enumerate(live):
                qf: QFormer = getattr(self, f"{m}_Qformer")
                # the modality with the most work is the step's critical path: its launches go first when both streams are ready
                with lane(m, high_priority=self.prioritize_heavy and pos == 0, after=heavy_done if pos > 0 else None) as hand:
                    enc, raw = self._qformer_input(qf, embeds[m], None if index is None else index.get(m), n_local)
                    res = qf.forward_fused(ids, att, enc, want_query=True, want_full=want_full, want_cls=True,
                                           kv_events=(self.roofline_events or {}).get(m), raw=raw)
                    z, cls = res["query"], res["cls"]
                    hand((enc, z, cls))
                    if sharded:      # scored after ONE packed all-gather of every modality's rows, below
                        local[m] = (z, cls)
                        if want_full:
                            out["full"][m] = self._gather(res["full"], n)
                            hand((out["full"][m],))
                        continue
                    hand(_store_scores(out, m, z, cls))
                    if want_full:
                        out["full"][m] = res["full"]
                        hand((res["full"],))
                    if want_llm:
                        hand(self._pack_llm(out, m, z, bs, num))
        if sharded and local:
            # the only exchange of the path: query embeddings and [CLS] vectors of all modalities in one RCCL all-gather
            mods_l = list(local)
            gathered = parallel.all_gather_packed([t for m in mods_l for t in local[m]], n, self.process_group)
            for k, m in enumerate(mods_l):
                _store_scores(out, m, gathered[2 * k], gathered[2 * k + 1])
                if want_llm:
                    self._pack_llm(out, m, out["z"][m], bs, num)
        mods = [m for m in self.modalities if m in out["logit"]]
        if not mods:
            raise MraError("no features for any of the model's modalities")
        # (sharded: on the gathered logits, so every rank ranks the same windows)
        out.update(self._score_tail([out["logit"][m] for m in mods], bs, num))
        out["bs"], out["num"] = bs, num
        return out

    def _pair_ok(self, live) -> bool:
        """The two live modalities can share one launch sequence: equal Q-Former shapes, operand-dtype score chain (automatic precision
        only once it resolved to op), no streaming fold."""
        a, b = (getattr(self, f"{m}_Qformer").cfg for m in live)
        same = all(getattr(a, k) == getattr(b, k) for k in ("hidden", "heads", "inter", "layers", "cross_freq", "n_query", "op_dtype"))

        def op_chain(qf) -> bool:
            mode = getattr(qf, "_cross_precision", "op")
            return mode == "op" or (mode == "auto" and qf.cross_precision_report()["resolved"] == "op")

        return same and all(op_chain(getattr(self, f"{m}_Qformer")) and getattr(getattr(self, f"{m}_Qformer"), "_cross_mode", "auto") != "fold_stream"
                            for m in live)

    def cross_precision_report(self) -> Dict[str, dict]:
        """Per modality ``QFormer.cross_precision_report()``: the precision mode set, the one in force and the measured attention sharpness."""
        return {m: getattr(self, f"{m}_Qformer").cross_precision_report() for m in self.modalities}

    @torch.no_grad()
    def encode_fuse(self, samples, want_llm: bool = False, want_full: bool = False) -> Dict[str, object]:
        """The seam ``generate`` and ``forward`` share (reference ``:228-306`` / ``:409-478``).

        Returns ``z[m]`` [N,32,768] (= ``last_hidden_state[:, :32]``), ``cls[m]`` [N,768], ``sim[m]``
        [N,32], ``logit[m]`` [N], ``fused`` [N], ``spans`` int32 [B,2]; with ``want_llm`` also
        ``inputs_llm[m]`` [B, T*32, 4096] and ``atts_llm[m]`` (``:303-306``).  With a process group the
        items are sharded in contiguous blocks over the ranks (every rank is given the same samples)."""
        ids, tmask = self._tokenize(samples["text_input"])
        rank, ws = self._clip_world()
        embeds, index = {}, {}
        bs = num = None
        for m in self.modalities:
            if not self._present(samples, m):
                continue
            src = samples.get(f"{m}_embeds", samples.get(m))
            if src is None and m == "video":   # video as decoded bytes: B clips x the processor's frames
                n_items = len(samples["video_raw"]) * int(getattr(self.video_processor, "n_frms", 0))
            elif src is None:    # audio as raw waveforms: B clips x the processor's temporal positions
                n_items = len(samples["audio_wave"]) * int(getattr(self.audio_processor, "n_frames", 0))
            else:
                n_items = int(src.shape[0]) * int(src.shape[2] if (m == "video" and f"{m}_embeds" not in samples) else src.shape[1])
            lo, hi = parallel.shard_range(n_items, rank, ws)
            embeds[m], _, bs, num = self._encode(samples, m, lo, hi)     # this rank's block only: the encoder is sharded too
        if bs is None:
            raise MraError("samples holds none of the model's modalities")
        # (fuse_score puts the query-token ones in front of this rank's rows of the mask)
        ids_n, tm_n = _expand_rows(ids, num, tile=self.compat_repeat), _expand_rows(tmask, num, tile=self.compat_repeat)
        lo, hi = parallel.shard_range(bs * num, rank, ws)
        return self.fuse_score(embeds, ids_n[lo:hi], tm_n[lo:hi], bs, num, index=index or None, want_llm=want_llm, want_full=want_full)

    @torch.no_grad()
    def generate(self, samples) -> List[str]:
        """Reference ``:221-397`` with the LLM decode replaced by the scorer: one ``"[[start, end]]"``
        string (seconds) per sample."""
        out = self.encode_fuse(samples)
        return _span_texts(out["spans"], _timestamps(samples, out["bs"], out["num"]))

    @torch.no_grad()
    def generate_with_scores(self, samples):
        """``generate`` plus the fused per-position logits ``[B][T]`` the spans were cut from (the
        ``pred_saliency_scores`` of the highlight metrics, ``eval/mr_eval.py:291-325``)."""
        out = self.encode_fuse(samples)
        scores = out["fused"].view(out["bs"], out["num"]).float().cpu().tolist()
        return _span_texts(out["spans"], _timestamps(samples, out["bs"], out["num"])), scores

    @torch.no_grad()
    def generate_windows(self, samples):
        """Ranked proposals (needs ``top_k > 1``): ``(texts, records, saliency)`` with per sample the
        ``"[[a, b], [c, d]]"`` string, the ``[start_s, end_s, score]`` triples in rank order (the
        ``pred_relevant_windows`` that ``eval/mr_eval.py:21-94`` scores) and the fused logits ``[T]``."""
        if self.top_k <= 1:
            raise MraError("generate_windows needs a model built with top_k > 1")
        out = self.encode_fuse(samples)
        texts, records = _window_texts(out["windows"], out["window_scores"], out["window_counts"], _timestamps(samples, out["bs"], out["num"]))
        saliency = out["fused"].view(out["bs"], out["num"]).float().cpu().tolist()
        return texts, records, saliency

    # ---- several queries per video over one shared K/V cache ---------------------------------------------------
    def _multi_pack(self, flat: Dict[str, object], logit: Dict[str, torch.Tensor], bs: int, num: int, P: int, counts: Sequence[int]) -> Dict[str, object]:
        """Per-video views of the (b, p, t)-ordered results of ``bs * P`` scored rows, the padded prompt slots dropped."""
        out: Dict[str, object] = {"bs": bs, "num": num, "counts": list(counts)}
        out["fused"] = [flat["fused"].view(bs, P, num)[b, :c] for b, c in enumerate(counts)]
        out["spans"] = [flat["spans"].view(bs, P, 2)[b, :c] for b, c in enumerate(counts)]
        out["logit"] = {m: [x.view(bs, P, num)[b, :c] for b, c in enumerate(counts)] for m, x in logit.items()}
        if "windows" in flat:
            k = self.top_k
            out["windows"] = [flat["windows"].view(bs, P, k, 2)[b, :c] for b, c in enumerate(counts)]
            out["window_scores"] = [flat["window_scores"].view(bs, P, k)[b, :c] for b, c in enumerate(counts)]
            out["window_counts"] = [flat["window_counts"].view(bs, P)[b, :c] for b, c in enumerate(counts)]
        return out

    def _multi_op_chain(self, qf: QFormer, ids_one: torch.Tensor, att_one: torch.Tensor, enc_one: torch.Tensor) -> bool:
        """Whether ``qf`` runs the operand-dtype score chain (what ``forward_multi`` needs).  Automatic precision that has not been
        resolved yet is resolved here, once, by an ordinary forward on one video and one query."""
        mode = getattr(qf, "_cross_precision", "op")
        if mode == "auto" and qf.cross_precision_report()["resolved"] is None:
            qf.forward_fused(ids_one, att_one, enc_one, want_query=True)
        return mode == "op" or (mode == "auto" and qf.cross_precision_report()["resolved"] == "op")

    def _multi_forward(self, qf: QFormer, m: str, ids_n: torch.Tensor, att: torch.Tensor, enc: torch.Tensor, P: int, num: int,
                       want_cls: bool = True):
        """The inference forward of ``P`` prompt slots per item: ``(z [items * P, 32, H], cls [items * P, H] or None)`` in (item, slot)
        row order.  ``forward_multi`` over one shared K/V cache; where split precision is in force one ordinary forward per slot."""
        if self._multi_op_chain(qf, ids_n[0:num * P:P], att[0:num * P:P], enc[:num]):
            res = qf.forward_multi(ids_n, att, enc, P, want_query=True, want_cls=want_cls)
            return res["query"], res.get("cls")
        if not getattr(self, "_multi_split_warned", False):
            logging.warning("encode_fuse_multi: split precision is in force for %s -- one ordinary forward per prompt slot, "
                            "no shared K/V cache", m)
            self._multi_split_warned = True
        items = int(enc.shape[0])
        per = [qf.forward_fused(ids_n[p::P], att[p::P], enc, want_query=True, want_cls=want_cls) for p in range(P)]
        z = torch.stack([r["query"] for r in per], dim=1).reshape(items * P, self.num_query_token, -1)
        cls = torch.stack([r["cls"] for r in per], dim=1).reshape(items * P, -1) if want_cls else None
        return z, cls

    @torch.no_grad()
    def encode_fuse_multi(self, samples, queries: Sequence[Sequence[str]]) -> Dict[str, object]:
        """``encode_fuse`` for several queries per video: ``queries[b]`` is the list of prompts of video ``b`` (ragged counts are
        padded to the largest count ``P`` by repeating the last prompt, and the padded results are dropped).  The encoders and the
        modality LayerNorm run once per video; each modality Q-Former runs ``forward_multi`` -- ``P`` prompts per position over
        ONE K/V projection -- on its own stream as in ``fuse_score``.  Prompts are always aligned to their own video: the
        reference's ``ids.repeat(num, 1)`` row order (``compat_repeat``) does not exist on this path.

        Returns ``fused`` (per video ``[P_b, T]``), ``spans`` (``[P_b, 2]``), with ``top_k > 1`` ``windows`` / ``window_scores`` /
        ``window_counts``, and ``logit[m]`` (per video ``[P_b, T]``).  One query per video for the whole call is ``encode_fuse`` itself
        (aligned prompts, the handle's cross mode).  Where split precision is in force (set, or resolved by the automatic mode) the
        modality falls back to one ordinary forward per prompt slot, with a warning.  Not sharded: a process group of more than one
        rank raises ``MraError``."""
        ranks = self._clip_world()[1]
        if ranks == 1 and callable(getattr(self.process_group, "size", None)):   # (a group handed over before torch.distributed is up)
            ranks = int(self.process_group.size())
        if ranks > 1:
            raise MraError("encode_fuse_multi is not sharded over a process group: run it on one rank")
        queries = [list(q) for q in queries]
        if not queries or any(len(q) == 0 for q in queries):
            raise MraError("encode_fuse_multi: every video needs at least one query")
        padded, counts = pad_queries(queries)
        P = max(counts)
        if P == 1:
            one = dict(samples)
            one["text_input"] = [q[0] for q in queries]
            keep, self.compat_repeat = self.compat_repeat, False
            try:
                res = self.encode_fuse(one)
            finally:
                self.compat_repeat = keep
            if res["bs"] != len(queries):
                raise MraError(f"encode_fuse_multi: {len(queries)} query lists for {res['bs']} videos")
            return self._multi_pack(res, res["logit"], res["bs"], res["num"], 1, counts)
        ids, tmask = self._tokenize([t for q in padded for t in q])      # [B * P, L], row b * P + p
        embeds = {}
        bs = num = None
        for m in self.modalities:
            if self._present(samples, m):
                embeds[m], _, bs, num = self._encode(samples, m)
        if bs is None:
            raise MraError("samples holds none of the model's modalities")
        if bs != len(queries):
            raise MraError(f"encode_fuse_multi: {len(queries)} query lists for {bs} videos")
        self._sync()
        # chain row (b * T + t) * P + p carries prompt p of video b
        ids_n, att = _prompt_rows(ids, tmask, self.num_query_token, num, P)
        live = [m for m in self.modalities if m in embeds]
        logit: Dict[str, torch.Tensor] = {}
        with self._modality_streams(self.overlap_modalities and len(live) > 1) as lane:
            for m in live:
                qf: QFormer = getattr(self, f"{m}_Qformer")
                with lane(m) as hand:
                    enc = qf.modality_ln(embeds[m].to(self._device))
                    z, cls = self._multi_forward(qf, m, ids_n, att, enc, P, num)
                    _, lg = scorer.cosine_scores(z, cls, want_sim=False)
                    # (b, t, p) -> (b, p, t): the scorer's heads then see bs * P "videos" of num positions
                    logit[m] = lg.index_select(0, bpt_index(bs, num, P).to(lg.device))
                    hand((enc, z, cls, lg, logit[m]))
        flat = self._score_tail([logit[m] for m in live], bs * P, num)
        return self._multi_pack(flat, logit, bs, num, P, counts)

    @torch.no_grad()
    def generate_multi(self, samples, queries: Sequence[Sequence[str]]) -> List[List[str]]:
        """``generate`` for several queries per video (``encode_fuse_multi``): per video one ``"[[start, end]]"`` string per query."""
        out = self.encode_fuse_multi(samples, queries)
        ts = _timestamps(samples, out["bs"], out["num"])
        return [_span_texts(sp, [t] * int(sp.shape[0])) for sp, t in zip(out["spans"], ts)]

    @torch.no_grad()
    def generate_multi_with_scores(self, samples, queries: Sequence[Sequence[str]]):
        """``generate_multi`` plus the fused per-position logits ``[B][P_b][T]`` the spans were cut from."""
        out = self.encode_fuse_multi(samples, queries)
        ts = _timestamps(samples, out["bs"], out["num"])
        texts = [_span_texts(sp, [t] * int(sp.shape[0])) for sp, t in zip(out["spans"], ts)]
        return texts, [f.float().cpu().tolist() for f in out["fused"]]

    @torch.no_grad()
    def generate_multi_windows(self, samples, queries: Sequence[Sequence[str]]):
        """``generate_windows`` for several queries per video (needs ``top_k > 1``): ``(texts, records, saliency)``, each ``[B][P_b]``."""
        if self.top_k <= 1:
            raise MraError("generate_multi_windows needs a model built with top_k > 1")
        out = self.encode_fuse_multi(samples, queries)
        ts = _timestamps(samples, out["bs"], out["num"])
        per_video = [_window_texts(win, sc, cnt, [t] * int(win.shape[0]))
                     for win, sc, cnt, t in zip(out["windows"], out["window_scores"], out["window_counts"], ts)]
        return [texts for texts, _ in per_video], [records for _, records in per_video], [f.float().cpu().tolist() for f in out["fused"]]

    # ---- row N2: the reference's own decode, for callers that attach a stock LLM ----------------------------
    def attach_llm(self, llm_model: nn.Module, llm_tokenizer, enumerate_inputs: bool = False, interleave_seconds: bool = True) -> None:
        """Attach a stock causal LM (``LlamaForCausalLM`` in the reference, ``:146-172``) and its tokenizer.  The hot
        path then feeds it exactly as the reference does (``models/llm_prompt.py``); the LM runs as ordinary
        PyTorch-ROCm.  Kept outside ``state_dict`` (the reference checkpoints hold the LLM separately)."""
        from .llm_prompt import PromptAssembler

        object.__setattr__(self, "llm_model", llm_model)
        self.llm_tokenizer = llm_tokenizer
        emb = llm_model.get_input_embeddings()
        if emb.weight.shape[1] != self.llm_hidden_size:
            raise MraError(f"LLM hidden size {emb.weight.shape[1]} != llm_hidden_size {self.llm_hidden_size} of the projections")
        self.prompt_assembler = PromptAssembler(llm_tokenizer, emb, modalities=self.modalities, num_query_token=self.num_query_token,
                                                enumerate_inputs=enumerate_inputs, interleave_seconds=interleave_seconds,
                                                max_txt_len=self.max_txt_len, max_output_txt_len=self.max_output_txt_len, device=self._device)

    def enable_lora(self, r: int = 8, alpha: float = 8, dropout: float = 0.05) -> None:
        """LoRA adapters on every linear of the attached LM except ``lm_head`` -- the reference's own trainable set (``:147-165``,
        ``models/model_utils.py``; ``models/lora.py`` here).  Needs ``attach_llm`` first; a second call changes nothing.  The adapters are
        the LM's parameters: outside ``state_dict()``, listed by ``lora_parameters()``, saved by the trainer under ``llm_model.*``.  With
        ``objective`` "llm" / "both" the Q-Formers may then stay frozen (the reference's regime): the Q-Former side runs without grad and the
        loss is differentiable with respect to the adapters; with ``enable_qformer_training()`` as well everything trains together."""
        from .lora import apply_lora, lora_modules

        if self.llm_model is None:
            raise MraError("no LLM attached: call attach_llm(llm_model, llm_tokenizer) first")
        if self.lora:
            return
        apply_lora(self.llm_model, r=r, alpha=alpha, dropout=dropout)
        self._lora_mods = list(lora_modules(self.llm_model).values())
        if not self._lora_mods:
            raise MraError("the attached LM has no nn.Linear to adapt")
        self.lora = True
        for mod in self._lora_mods:
            mod.train(self.training)

    def lora_parameters(self) -> List[nn.Parameter]:
        from .lora import lora_parameters

        return lora_parameters(self.llm_model) if self.lora else []

    def train(self, mode: bool = True):
        """The attached LM is not a submodule and keeps its own mode; its adapters follow this model's (their dropout is a training-mode op)."""
        nn.Module.train(self, mode)
        if self.lora:
            for mod in self._lora_mods:
                mod.train(mode)
        return self

    def _lora_loss(self, loss: torch.Tensor) -> torch.Tensor:
        """With the Q-Formers frozen the LM loss reaches only the adapters: its gradient carries ``loss_scale`` into the LM here (with the
        Q-Formers training ``_lm_loss`` does it) and every ``LoraLinear`` divides it out of its adapter gradients in fp32."""
        return _ScaleGrad.apply(loss, float(self.loss_scale)) if self.loss_scale != 1.0 and loss.requires_grad else loss

    def _lora_unscale(self) -> None:
        if self.lora:
            for mod in self._lora_mods:
                mod.grad_unscale = 1.0 / float(self.loss_scale)

    def _lm_ce(self, embeds, mask, targets):
        """The LM's cross-entropy on the answer tokens.  ``lm_loss = "stock"``: the LM's own forward with ``labels`` (the reference's call,
        ``:599-604``; ``lm_head`` runs over every position).  ``"rows"`` / ``"fused"``: the LM's decoder alone, then ``lm_head_ce`` on the
        final hidden states -- the head and the loss on the labelled rows only, as torch ops or on the HIP entries; ``lm_head`` itself is
        never called, so its weight gets no gradient under ``"fused"`` (the reference never trains it).  ``lm_attention = "hip"``: the same
        call, on any of the three routes, inside ``lm_attention.hip_train``."""
        lm_attention = getattr(self, "lm_attention", "stock")
        if lm_attention == "stock":
            return _lm_ce_call(self, embeds, mask, targets)
        if lm_attention not in LM_ATTENTIONS:
            raise MraError(f"lm_attention must be 'stock' or 'hip', got {lm_attention!r}")
        from .lm_attention import hip_train, hold_for_backward

        with hip_train(self.llm_model):
            loss = _lm_ce_call(self, embeds, mask, targets)
        return hold_for_backward(self.llm_model, loss)       # activation checkpointing: the recomputation runs the same attention

    def _llm_inputs(self, samples):
        if self.prompt_assembler is None:
            raise MraError("no LLM attached: call attach_llm(llm_model, llm_tokenizer) first")
        with torch.no_grad():
            out = self.encode_fuse(samples, want_llm=True)
        if self.prompt_assembly == "plan":      # the gather reads the fp32 projections themselves and casts them
            return out["inputs_llm"], out["atts_llm"]
        dt = self.llm_model.get_input_embeddings().weight.dtype
        return {m: v.to(dt) for m, v in out["inputs_llm"].items()}, out["atts_llm"]

    def _plan_assemble(self, samples, media: Dict[str, torch.Tensor], generate: bool = False, first_rows=None):
        """The plan route: ``(embeds, mask, targets)`` of ``samples`` (one prompt per sequence) over the projections ``media[m]``, whose
        row ``first_rows[seq, pos] + q`` is query ``q`` of sequence ``seq`` at position ``pos`` (default: the ordinary ``[B, T * 32, D]``
        layout).  ``media`` stays in its own dtype: the cast to the LM's dtype happens inside the gather."""
        from .llm_prompt import assemble_plan

        asm, Q = self.prompt_assembler, self.num_query_token
        mods = [m for m in asm.modalities if m in media]
        rows = {m: media[m].numel() // media[m].shape[-1] for m in mods}
        num = None if first_rows is not None else rows[mods[0]] // (Q * len(samples["text_input"]))
        build = asm.plan_generate if generate else asm.plan_forward
        plan = build(samples, first_rows, Q, num=int(first_rows.shape[1]) if first_rows is not None else num, rows=rows, modalities=mods)
        out = assemble_plan(plan, self.llm_model.get_input_embeddings().weight, {m: media[m] for m in mods})
        return (*out, plan)

    @torch.no_grad()
    def generate_llm(self, samples, max_new_tokens: int = 64) -> List[str]:
        """Reference ``generate`` end to end (``:221-397``): hot path -> prompt assembly -> ``llm_model.generate``."""
        inputs_llm, atts_llm = self._llm_inputs(samples)
        if self.prompt_assembly == "plan":
            embeds, mask, _, _ = self._plan_assemble(samples, inputs_llm, generate=True)
        else:
            embeds, mask = self.prompt_assembler.assemble_generate(samples, inputs_llm, atts_llm)
        return self._llm_decode(embeds, mask, max_new_tokens)

    def _llm_decode(self, embeds, mask, max_new_tokens: int) -> List[str]:
        """``lm_decode = "stock"``: the reference's call.  ``"hip"``: the same greedy decode over a static cache (no ``torch.cat`` of the K/V per
        token) with every one-token attention on ``mra_decode_attention`` (``models/lm_decode.py``); ``disable_compile`` because ``generate``
        would otherwise compile the forward around the ctypes launches.  ``"hip_step"``: the prefill through the LM's own forward, then one
        ``mra_lm_step`` per token (``models/lm_step.py``: weight-streaming layers, head and greedy bookkeeping on HIP).  ``lm_prefill = "hip"``
        (with either HIP decode): the prefill's attention on ``mra_prefill_attention``.  The LM is as it was after the call."""
        lm_prefill = getattr(self, "lm_prefill", "stock")
        check_lm_options(self.lm_decode, lm_prefill, unknown_decode=MraError)
        if self.lm_decode == "stock":
            outputs = self.llm_model.generate(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=max_new_tokens)
        elif self.lm_decode == "hip":
            from .lm_decode import hip_decode

            with hip_decode(self.llm_model, prefill=lm_prefill == "hip"):
                outputs = self.llm_model.generate(inputs_embeds=embeds, attention_mask=mask, max_new_tokens=max_new_tokens,
                                                  cache_implementation="static", disable_compile=True)
        else:                                                          # "hip_step"
            from .lm_step import HipLmDecoder

            dec = getattr(self, "_lm_stepper", None)
            if dec is None or dec.llm is not self.llm_model or dec.prefill != lm_prefill:
                dec = self._lm_stepper = HipLmDecoder(self.llm_model, prefill=lm_prefill)
            outputs = dec.generate(embeds, mask, max_new_tokens)
        outputs[outputs == 0] = 2                                      # :392
        return [o.strip() for o in self.llm_tokenizer.batch_decode(outputs, skip_special_tokens=True)]

    @torch.no_grad()
    def generate_multi_llm(self, samples, queries: Optional[Sequence[Sequence[str]]] = None, max_new_tokens: int = 64) -> List[List[str]]:
        """``generate_llm`` for several queries per video: per video one decoded string per query.  The frozen route of the grouped pass
        (``forward_multi`` per modality over one K/V projection per video, calls of at most ``max_queries_per_call`` prompt slots), the
        projections in ``(video, position, prompt)`` row order as they come, ``plan_generate`` and ``llm_model.generate`` on one LM batch
        per call holding its real ``(video, query)`` sequences."""
        if self.prompt_assembler is None:
            raise MraError("no LLM attached: call attach_llm(llm_model, llm_tokenizer) first")
        queries = [list(q) for q in (queries if queries is not None else samples["text_input"])]
        if not queries or any(len(q) == 0 for q in queries):
            raise MraError("generate_multi_llm: every video needs at least one query")
        texts: List[List[str]] = [[] for _ in queries]
        for call in self._multi_calls(samples, queries, train=False, want_cls=False):
            flat, first = self._multi_flatten(samples, queries, None, call)
            media = {m: getattr(self, f"{m}_Qformer").llm_proj(z) for m, (z, _) in call["out"].items()}
            embeds, mask, _, _ = self._plan_assemble(flat, media, generate=True, first_rows=first)
            for (k, _), txt in zip(call["pairs"], self._llm_decode(embeds, mask, max_new_tokens)):
                texts[call["vids"][k]].append(txt)
        return texts

    def _check_lm_training(self) -> None:
        if self.prompt_assembler is None:
            raise MraError("no LLM attached: call attach_llm(llm_model, llm_tokenizer) first")
        if not getattr(self, "train_qformers", False):
            raise MraError("the LM objective trains the Q-Formers: call enable_qformer_training() first")

    def _check_grouped_lm(self) -> None:
        """The LM objective on a grouped batch is opt-in like every other switch here: with the default a grouped batch under an LM
        objective is refused exactly as before."""
        if not getattr(self, "grouped_lm", False):
            raise MraError(f"objective {self.objective!r} on a grouped batch: the multi-query LM pass is off -- switch it on with "
                           "XInstructBLIP(grouped_lm=True) / model.grouped_lm = True (Trainer does, for group_by_video with an LM objective), "
                           "or train grouped batches with objective 'score'")

    def forward_llm(self, samples, train: Optional[bool] = None):
        """Reference ``forward`` end to end (``:399-606``): the LM's cross-entropy on the answer tokens.  ``train=False``: the
        Q-Former side is computed without grad (frozen, as in the reference); the loss trains whatever the LM leaves trainable.
        ``train=True`` (default: ``objective != "score"`` after ``enable_qformer_training()``): the loss is differentiable with
        respect to the Q-Formers, the query tokens, ``{m}_ln`` under ``train_ln`` and ``{m}_llm_proj`` under ``train_proj`` -- the
        BLIP-2 stage-2 / InstructBLIP recipe with a frozen LM.  Encoders run under ``no_grad``; the Q-Former text rows follow
        ``forward`` (``compat_repeat``).  The LM is never modified: whatever it leaves trainable still receives gradients.
        A 16-bit LM's activation gradients are 16-bit too and the LM loss is a mean over the answer tokens, so with an f16 LM the small
        ones flush to zero before they reach the projection: use bf16, or set ``loss_scale`` (e.g. 1024): the LM term's gradient is
        multiplied by it going into the LM and divided out in fp32 inside the projection's backward, so the loss value and the
        gradients of the projections, Q-Formers and LayerNorms are unscaled.  Gradients of parameters INSIDE the LM are then
        ``loss_scale`` times too large (divide them yourself): a frozen LM is the intended use.  The LoRA adapters of ``enable_lora()`` are
        the exception: each ``LoraLinear`` divides the scale out of its own gradients in fp32, so adapter ``.grad``s are unscaled.  With
        LoRA on and the Q-Formers frozen, ``train=False`` is the training route (the reference's regime)."""
        if train is None:
            train = self.objective != "score" and getattr(self, "train_qformers", False)
        if _is_grouped(samples):           # one record per video with the lists of its queries: forward_multi's pass, the LM term alone
            if train:
                self._check_lm_training()
            elif self.prompt_assembler is None:
                raise MraError("no LLM attached: call attach_llm(llm_model, llm_tokenizer) first")
            self._check_grouped_lm()
            return {"loss": self._multi_losses(samples, None, None, want_score=False, want_llm=True, train=bool(train))["lm"]}
        if train:
            self._check_lm_training()
            _, inputs_llm, _, _ = self._train_pass(samples, want_score=False, want_llm=True)
            return {"loss": self._lm_loss(samples, inputs_llm)}
        inputs_llm, atts_llm = self._llm_inputs(samples)
        if getattr(self, "prompt_assembly", "cat") == "plan":
            embeds, mask, targets, _ = self._plan_assemble(samples, inputs_llm)
        else:
            embeds, mask, targets = self.prompt_assembler.assemble_forward(samples, inputs_llm, atts_llm)
        self._lora_unscale()
        loss = self._lm_ce(embeds, mask, targets)
        return {"loss": self._lora_loss(loss) if self.lora else loss}

    _WINDOW = re.compile(r"\[\s*(-?\d+(?:\.\d+)?)\s*,\s*(-?\d+(?:\.\d+)?)\s*\]")

    @classmethod
    def parse_windows(cls, txt: str) -> List[List[float]]:
        """``text_output`` of the reference's datasets (``utils/mr_dataset.py:100-106``): ``"[[s, e]]"`` or several
        windows ``"[[s0, e0], [s1, e1]]"`` (QVHighlights), integer or float seconds (``save_float=True`` in the
        reference's preprocessing).  Returns every ``[start, end]`` pair; ``[[-1, -1]]`` (no window) gives ``[]``.
        Raises on text with no window at all, so a malformed annotation cannot silently train on an empty target."""
        wins = [[float(a), float(b)] for a, b in cls._WINDOW.findall(txt)]
        if not wins:
            raise ValueError(f"text_output holds no [start, end] window: {txt!r}")
        return [[min(a, b), max(a, b)] for a, b in wins if a >= 0 and b >= 0]

    def _targets(self, samples, bs, num):
        """Clip-membership targets: position ``i`` of sample ``r`` is positive when its timestamp lies inside ANY of
        the windows of ``samples["text_output"][r]`` (union over windows, float seconds honoured)."""
        target = torch.zeros(bs, num, dtype=torch.float32, device=self._device)
        ts = _timestamps(samples, bs, num)
        for r, txt in enumerate(samples.get("text_output", ["[[-1, -1]]"] * bs)):
            _membership_targets(self.parse_windows, [txt], ts[r], target[r: r + 1])
        return target

    def enable_qformer_training(self, train_ln: bool = False, train_proj: bool = False) -> None:
        """Unfreeze the Q-Formers (the reference keeps them frozen, ``:196-204``; BASELINE config 5 trains
        them): parameters get ``requires_grad`` and gradients from the HIP backward.  ``train_ln``: the modality
        LayerNorms ``{m}_ln`` in front of them are trained too (``QFormer.modality_ln_train``: the encoder-side data
        gradient of the Q-Former and the LayerNorm backward run on the HIP extension); they stay ordinary torch
        parameters, which ``flat_optimizer_params`` lists behind the flat ones.  ``train_proj``: likewise the projections
        ``{m}_llm_proj`` into the LM (``QFormer.llm_proj_train``, ``mra_llm_proj_backward``), which only the LM objectives
        (``objective`` "llm" / "both") reach.  The default leaves the step as it is."""
        self.train_qformers = True
        self.train_ln = bool(train_ln)
        self.train_proj = bool(train_proj)

        def ln_dirty():
            self._extras_dirty = True          # fused optimizers do not bump version counters (see QFormer._run_backward)

        for m in self.modalities:
            if self.train_ln:
                for p in getattr(self, f"{m}_ln").parameters():
                    p.requires_grad_(True)
            if self.train_proj:
                for p in getattr(self, f"{m}_llm_proj").parameters():
                    p.requires_grad_(True)
            getattr(self, f"{m}_Qformer")._ln_grad_hook = ln_dirty if self.train_ln else None
            getattr(self, f"{m}_Qformer")._proj_grad_hook = ln_dirty if self.train_proj else None
        for m in self.modalities:
            qf: QFormer = getattr(self, f"{m}_Qformer")
            qf.enable_training()
            qt = getattr(self, f"{m}_query_tokens")
            qt.requires_grad_(True)

            # the query tokens live in the Q-Former's flat master / gradient buffers too (slot "query_tokens")
            off, numel = qf._slice_of("query_tokens")
            with torch.no_grad():
                view = qf._master_flat[off: off + numel].view_as(qt)
                view.copy_(qt.data)
                qt.data = view

            def binder(qf=qf, qt=qt):
                qt.grad = qf.grad_of("query_tokens").view_as(qt)
                self._extras_dirty = True      # fused optimizers do not bump version counters (see QFormer._run_backward)

            qf._extra_grad_binder = binder

    def forward(self, samples):
        """Reference ``:399-606`` returns the LLM's cross-entropy.  Without an LLM on this path the
        training signal is build-defined: binary cross-entropy between sigmoid(20 * fused logit) and clip
        membership of the target span parsed from ``text_output``.  After ``enable_qformer_training()`` the
        loss is differentiable w.r.t. every Q-Former parameter (forward + backward on the HIP extension; the
        few-KB scorer and the loss run as torch ops so autograd can seed the backward); otherwise it is a
        forward-only value, as the reference's frozen Q-Formers would give."""
        if samples is None or samples == {} or not any(self._present(samples, m) for m in self.modalities):
            return {"loss": torch.tensor(0.0)}
        ti = samples.get("text_input")
        grouped = ti is not None and len(ti) > 0 and isinstance(ti[0], (list, tuple))
        if self.objective != "score":
            if self.objective not in ("llm", "both"):
                raise MraError(f"objective must be 'score', 'llm' or 'both', got {self.objective!r}")
            if grouped:
                self._check_grouped_lm()
            frozen = self.lora and not getattr(self, "train_qformers", False)     # the reference's regime: only the adapters train
            if self.objective == "llm":
                return self.forward_llm(samples, train=not frozen)
            if grouped:    # forward_multi's BCE and the LM term over ONE Q-Former forward (and backward) per modality and call
                if not frozen:
                    self._check_lm_training()
                out = self._multi_losses(samples, None, None, want_score=True, want_llm=True, train=not frozen)
                bce, lm = out["score"], out["lm"]
                return {"loss": bce + self.lm_weight * lm, "loss_score": bce.detach(), "loss_lm": lm.detach()}
            if frozen:
                with torch.no_grad():
                    out = self.encode_fuse(samples, want_llm=True)
                    bce = nn.functional.binary_cross_entropy_with_logits(out["fused"].view(out["bs"], out["num"]) * 20.0,
                                                                         self._targets(samples, out["bs"], out["num"]))
                if getattr(self, "prompt_assembly", "cat") == "plan":
                    embeds, mask, targets, _ = self._plan_assemble(samples, out["inputs_llm"])
                else:
                    dt = self.llm_model.get_input_embeddings().weight.dtype
                    embeds, mask, targets = self.prompt_assembler.assemble_forward(samples, {m: v.to(dt) for m, v in out["inputs_llm"].items()},
                                                                                   out["atts_llm"])
                self._lora_unscale()
                lm = self._lora_loss(self._lm_ce(embeds, mask, targets))
                return {"loss": bce + self.lm_weight * lm, "loss_score": bce.detach(), "loss_lm": lm.detach()}
            self._check_lm_training()
            per_mod, inputs_llm, bs, num = self._train_pass(samples, want_score=True, want_llm=True)
            bce, lm = self._score_loss(samples, per_mod, bs, num), self._lm_loss(samples, inputs_llm)
            return {"loss": bce + self.lm_weight * lm, "loss_score": bce.detach(), "loss_lm": lm.detach()}
        if grouped:   # one record per video with the list of its queries
            return self.forward_multi(samples)
        if not getattr(self, "train_qformers", False):
            out = self.encode_fuse(samples)
            bs, num = out["bs"], out["num"]
            logits = out["fused"].view(bs, num) * 20.0
            return {"loss": nn.functional.binary_cross_entropy_with_logits(logits, self._targets(samples, bs, num))}
        per_mod, _, bs, num = self._train_pass(samples, want_score=True, want_llm=False)
        return {"loss": self._score_loss(samples, per_mod, bs, num)}

    def _score_loss(self, samples, per_mod, bs, num):
        fused = _weighted_fuse(per_mod, self.fuse_weights)
        return nn.functional.binary_cross_entropy_with_logits(fused.view(bs, num) * 20.0, self._targets(samples, bs, num))

    def _train_pass(self, samples, want_score: bool, want_llm: bool):
        """ONE training forward per modality Q-Former (``forward_train``), connected to autograd, feeding what the objective asks for:
        ``want_score`` the per-position scorer logits ``max_q cos(z, cls)``, ``want_llm`` the projections into the LM
        ``inputs_llm[m]`` [B, T * 32, D] (fp32; ``llm_proj_train``, always a node: the Q-Former gets its gradient whether or not the
        projection is trained).  Returns ``(per_mod, inputs_llm, bs, num)``."""
        self._sync()
        ids, tmask = self._tokenize(samples["text_input"])
        per_mod, inputs_llm, bs, num = [], {}, None, None
        # ``train_streams``: each modality's forward (and, since autograd runs a node's backward on its forward's stream, its backward)
        # on its own stream.  Round 2 measured nothing from it (17.4 vs 17.0 ms: the step was bound by the GPU time of its ~1300 launches);
        # measured again after the launch merges of round 3 -- see DESIGN.md section 8.
        with self._modality_streams(bool(getattr(self, "train_streams", False))) as lane:
            for m in self.modalities:
                if not self._present(samples, m):
                    continue
                qf: QFormer = getattr(self, f"{m}_Qformer")
                with lane(m) as hand:
                    with torch.no_grad():
                        raw, idx, bs, num = self._encode(samples, m)
                    enc = self._train_norm(m, raw, idx, bs * num)
                    ids_n, att = _prompt_rows(ids, tmask, self.num_query_token, num, tile=self.compat_repeat)
                    z, cls = qf.forward_train(ids_n, att, enc, want_cls=want_score)
                    hand((enc, z, cls))
                    if want_score:
                        per_mod.append(_train_logit(z, cls))
                        hand(per_mod[-1:])
                    if want_llm:  # reference :303-306
                        proj = getattr(self, f"{m}_llm_proj")
                        y = qf.llm_proj_train(z, proj.weight, proj.bias, grad_scale=self.loss_scale)
                        inputs_llm[m] = y.reshape(bs, num * self.num_query_token, -1)
                        hand((inputs_llm[m],))
        return per_mod, inputs_llm, bs, num

    def _lm_loss(self, samples, inputs_llm):
        """The attached LM's cross-entropy on the answer tokens over differentiable ``inputs_llm`` (``PromptAssembler.assemble_forward`` is
        plain ``torch.cat``; ``prompt_assembly = "plan"`` is one gather node).  The value is the loss itself; only its gradient carries
        ``loss_scale`` into the LM."""
        if self.prompt_assembly == "plan":      # one gather node: no .to(dt) copies, the gradient comes back fp32 in one launch per modality
            embeds, mask, targets, _ = self._plan_assemble(samples, inputs_llm)
        else:
            dt = self.llm_model.get_input_embeddings().weight.dtype
            atts = {m: torch.ones(v.shape[0], v.shape[1], dtype=torch.long, device=self._device) for m, v in inputs_llm.items()}
            embeds, mask, targets = self.prompt_assembler.assemble_forward(samples, {m: v.to(dt) for m, v in inputs_llm.items()}, atts)
        self._lora_unscale()
        loss = self._lm_ce(embeds, mask, targets)
        return _ScaleGrad.apply(loss, float(self.loss_scale)) if self.loss_scale != 1.0 else loss

    def _ln_train(self, m: str, raw: torch.Tensor) -> torch.Tensor:
        """``{m}_ln`` over the encoder output as an autograd node (``enable_qformer_training(train_ln=True)``)."""
        ln = getattr(self, f"{m}_ln")
        return getattr(self, f"{m}_Qformer").modality_ln_train(raw.to(self._device), ln.weight, ln.bias)

    max_queries_per_call = 8      # forward_multi: most queries of one video in one Q-Former call (the backward core's LDS holds 14)

    def _multi_targets(self, samples, windows: Sequence[Sequence[str]], num: int) -> List[torch.Tensor]:
        """Per video ``[P_b, T]`` clip-membership targets: row ``p`` from the windows of the video's query ``p`` (as ``_targets``)."""
        ts = _timestamps(samples, len(windows), num)
        return [_membership_targets(self.parse_windows, txts, ts[b], torch.zeros(len(txts), num, dtype=torch.float32, device=self._device))
                for b, txts in enumerate(windows)]

    def forward_multi(self, samples, queries: Optional[Sequence[Sequence[str]]] = None, targets: Optional[Sequence[Sequence[str]]] = None):
        """``forward`` for one record per video with several queries: ``queries[b]`` / ``targets[b]`` are the prompts and the
        ``text_output`` strings of video ``b`` (default: the lists in ``samples["text_input"][b]`` / ``samples["text_output"][b]``).
        The loss is the binary cross-entropy of ``20 x fused logit`` against clip membership of each query's own windows, averaged
        over the real (video, query, position) triples -- the mean of the ``forward`` losses of one ``(video, query)`` sample each
        when every video has ``T`` positions.  The encoders and the modality LayerNorm run once per video under ``no_grad``; each
        modality Q-Former runs ``forward_multi_train``: ``P`` prompts per position over ONE K/V projection, one dK / dV tape and one
        K/V weight gradient.  Ragged counts are padded by ``pad_queries``; padded slots carry no loss and no gradient.  Videos
        with more than ``max_queries_per_call`` queries run as consecutive calls of at most that many, each call's loss weighted by
        its share of the triples.  Prompts are always aligned to their own video (no ``compat_repeat`` on this path).  Without
        ``enable_qformer_training()`` the loss is the forward-only value from ``encode_fuse_multi``.  The pass itself is ``_multi_calls``,
        which the LM objective on grouped batches (``forward`` / ``forward_llm`` with ``objective`` "llm" / "both") and
        ``generate_multi_llm`` share."""
        queries = [list(q) for q in (queries if queries is not None else samples["text_input"])]
        if targets is None:
            targets = samples.get("text_output") or [["[[-1, -1]]"] * len(q) for q in queries]
        targets = [list(t) for t in targets]
        if not queries or any(len(q) == 0 for q in queries):
            raise MraError("forward_multi: every video needs at least one query")
        if len(targets) != len(queries) or any(len(t) != len(q) for t, q in zip(targets, queries)):
            raise MraError("forward_multi: targets must hold one text_output per query")
        counts = [len(q) for q in queries]
        bce = nn.functional.binary_cross_entropy_with_logits
        if not getattr(self, "train_qformers", False):
            out = self.encode_fuse_multi(samples, queries)
            tg = self._multi_targets(samples, targets, out["num"])
            total = sum(bce(f.float() * 20.0, t, reduction="sum") for f, t in zip(out["fused"], tg))
            return {"loss": total / float(sum(counts) * out["num"])}
        out = self._multi_losses(samples, queries, targets, want_score=True, want_llm=False, train=True)
        return {"loss": out["score"] if out["score"] is not None else torch.tensor(0.0)}

    def _multi_calls(self, samples, queries: Sequence[Sequence[str]], train: bool, want_cls: bool):
        """The pass ``forward_multi``, the grouped LM objective and ``generate_multi_llm`` share, as a generator of calls.  Encoders and the
        modality LayerNorm once per video, then per call of at most ``max_queries_per_call`` prompt slots one Q-Former forward per modality:
        ``forward_multi_train`` when ``train`` (connected to autograd), else the inference ``forward_multi`` under ``no_grad`` (with its
        one-forward-per-slot fallback under split precision).  Yields ``vids`` (the videos that still have queries), ``cnt`` (their real
        counts in this call), ``lo``, ``P``, ``num``, ``pairs`` (the real ``(k, p)`` = (video slot, prompt slot) in order) and ``out[m] =
        (z, cls)`` in chain-row order ``(k * T + t) * P + p``.  Prompts are aligned to their own video."""
        step = int(self.max_queries_per_call)
        if step < 1:
            raise MraError("max_queries_per_call must be >= 1")
        counts = [len(q) for q in queries]
        self._sync()
        encs: Dict[str, torch.Tensor] = {}
        bs = num = None
        for m in self.modalities:
            if self._present(samples, m):
                with torch.no_grad():
                    raw, idx, bs, num = self._encode(samples, m)
                encs[m] = self._train_norm(m, raw, idx, bs * num)
        if bs is None:
            return
        if bs != len(queries):
            raise MraError(f"forward_multi: {len(queries)} query lists for {bs} videos")
        for lo in range(0, max(counts), step):
            vids = [b for b, c in enumerate(counts) if c > lo]            # the videos that still have queries in this round
            padded, cnt = pad_queries([queries[b][lo: lo + step] for b in vids])
            nb, P = len(vids), max(cnt)
            ids, tmask = self._tokenize([t for q in padded for t in q])      # [nb * P, L], row b * P + p
            # chain row (b * T + t) * P + p carries prompt p of video b
            ids_n, att = _prompt_rows(ids, tmask, self.num_query_token, num, P)
            sel = None if nb == bs else torch.as_tensor(vids, device=self._device)
            out = {}
            for m, enc in encs.items():
                if sel is not None:
                    enc = enc.view(bs, num, *enc.shape[1:]).index_select(0, sel).reshape(nb * num, *enc.shape[1:])
                qf: QFormer = getattr(self, f"{m}_Qformer")
                if train:
                    out[m] = qf.forward_multi_train(ids_n, att, enc, P, want_cls)
                else:
                    with torch.no_grad():
                        out[m] = self._multi_forward(qf, m, ids_n, att, enc, P, num, want_cls)
            yield {"vids": vids, "cnt": cnt, "lo": lo, "P": P, "num": num, "bs": bs, "out": out,
                   "pairs": [(k, p) for k in range(nb) for p in range(cnt[k])]}

    def _multi_flatten(self, samples, queries, targets, call):
        """One LM sequence per real ``(video, query)`` pair of a call: the flattened ``samples`` of ``PromptAssembler.plan_*`` and the table
        ``first [n_seq, T]`` of each sequence's first projection row per position in the call's ``(k, t, p)`` row order."""
        vids, lo, P, num, pairs = call["vids"], call["lo"], call["P"], call["num"], call["pairs"]
        ts = _timestamps(samples, call["bs"], num)
        flat = {"text_input": [queries[vids[k]][lo + p] for k, p in pairs], "timestamps": [ts[vids[k]] for k, _ in pairs],
                "duration": [samples["duration"][vids[k]] for k, _ in pairs]}
        if targets is not None:
            flat["text_output"] = [targets[vids[k]][lo + p] for k, p in pairs]
        kp = torch.tensor(pairs, dtype=torch.long)
        first = ((kp[:, 0, None] * num + torch.arange(num)[None, :]) * P + kp[:, 1, None]) * self.num_query_token
        return flat, first

    def _multi_losses(self, samples, queries, targets, want_score: bool, want_llm: bool, train: bool):
        """The loss terms of a grouped batch over ``_multi_calls``: ``score`` = ``forward_multi``'s BCE, ``lm`` = the attached LM's
        cross-entropy over all labelled answer tokens of all real ``(video, query)`` pairs -- per call one LM batch over the projections in
        ``(k, t, p)`` row order as they come (``llm_proj_train`` / ``llm_proj``, then the prompt plan), the calls combined with weights equal
        to their shares of the labelled tokens after the causal shift.  Both terms hang off ONE Q-Former forward per modality and call, so
        its backward runs once.  ``train`` False: the Q-Former side runs without grad (the frozen LoRA regime)."""
        queries = [list(q) for q in (queries if queries is not None else samples["text_input"])]
        if targets is None:
            targets = samples.get("text_output") or [["[[-1, -1]]"] * len(q) for q in queries]
        targets = [list(t) for t in targets]
        if not queries or any(len(q) == 0 for q in queries):
            raise MraError("forward_multi: every video needs at least one query")
        if len(targets) != len(queries) or any(len(t) != len(q) for t, q in zip(targets, queries)):
            raise MraError("forward_multi: targets must hold one text_output per query")
        counts = [len(q) for q in queries]
        bce = nn.functional.binary_cross_entropy_with_logits
        tg = score = None
        lm_parts = []
        for call in self._multi_calls(samples, queries, train, want_cls=want_score):
            vids, cnt, lo, P, num = call["vids"], call["cnt"], call["lo"], call["P"], call["num"]
            nb = len(vids)
            if want_score:
                if tg is None:
                    tg = self._multi_targets(samples, targets, num)
                    triples = float(sum(counts) * num)
                per_mod = [_train_logit(z, cls) for z, cls in call["out"].values()]
                fused = _weighted_fuse(per_mod, self.fuse_weights).view(nb, num, P).permute(0, 2, 1)      # (b, t, p) -> [nb, P, T]
                target = torch.zeros(nb, P, num, dtype=torch.float32, device=self._device)
                real = torch.zeros(nb, P, 1, dtype=torch.float32, device=self._device)                  # 0 on padded slots: no loss, no gradient
                for k, b in enumerate(vids):
                    target[k, :cnt[k]] = tg[b][lo: lo + cnt[k]]
                    real[k, :cnt[k]] = 1.0
                part = (bce(fused * 20.0, target, reduction="none") * real).sum() / triples
                score = part if score is None else score + part
            if want_llm:
                media = {}
                for m, (z, _) in call["out"].items():
                    qf, proj = getattr(self, f"{m}_Qformer"), getattr(self, f"{m}_llm_proj")
                    media[m] = qf.llm_proj_train(z, proj.weight, proj.bias, grad_scale=self.loss_scale) if train else qf.llm_proj(z)
                flat, first = self._multi_flatten(samples, queries, targets, call)
                embeds, mask, labels, plan = self._plan_assemble(flat, media, first_rows=first)
                probe = getattr(self, "_lm_probe", None)
                if probe is not None:          # tests look at what goes into the LM
                    probe({"call": call, "flat": flat, "media": media, "embeds": embeds, "mask": mask, "targets": labels})
                self._lora_unscale()
                loss = self._lm_ce(embeds, mask, labels)
                if train:
                    loss = _ScaleGrad.apply(loss, float(self.loss_scale)) if self.loss_scale != 1.0 else loss
                elif self.lora:
                    loss = self._lora_loss(loss)
                lm_parts.append((loss, int((plan.targets[:, 1:] != -100).sum())))
        lm = None
        if lm_parts:
            total = float(sum(n for _, n in lm_parts))
            for loss, n in lm_parts:
                part = loss if len(lm_parts) == 1 else loss * (n / total)
                lm = part if lm is None else lm + part
        return {"score": score, "lm": lm}

    def flat_optimizer_params(self) -> List[nn.Parameter]:
        """Parameters for an optimizer after ``enable_qformer_training()``: one flat parameter per Q-Former (bert.* and
        the query tokens are views of it) plus whatever else requires grad.  Same update as the per-tensor list."""
        covered, out = set(), []
        for m in self.modalities:
            qf: QFormer = getattr(self, f"{m}_Qformer")
            out.append(qf.flat_parameter())
            covered.update(id(p) for p in qf.parameters())
            covered.add(id(getattr(self, f"{m}_query_tokens")))
        out.extend(p for p in self.parameters() if p.requires_grad and id(p) not in covered)
        return out

    def all_reduce_grads(self) -> None:
        """Data-parallel gradient averaging over the process group: one all-reduce of each Q-Former's flat f32
        gradient buffer (what DDP does bucket by bucket in the reference's trainer, ``utils/trainer.py:69,133``).  Parameters outside
        the flat buffers (``{m}_ln.*`` under ``train_ln``, ``{m}_llm_proj.*`` under ``train_proj``) carry ordinary ``.grad`` tensors: ``Trainer._sync_grads`` averages those."""
        rank, ws = parallel.world(self.process_group)
        if ws == 1:
            return
        import torch.distributed as dist
        for m in self.modalities:
            flat = getattr(self, f"{m}_Qformer")._grad_flat
            dist.all_reduce(flat, group=self.process_group)
            flat.div_(ws)


def _ref(obj):
    import weakref
    return weakref.ref(obj)
