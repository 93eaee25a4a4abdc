"""BEATs audio encoder (row A1 callee, the audio half).

The reference builds it with LAVIS ``BeatsEncoder(checkpoint_path)`` (``models/xinstructblip.py:670-676``) and calls
``audio_encoder(fbank)`` once per clip position (``:267-275``); LAVIS' ``BeatsEncoder.forward`` is
``extract_features(fbank, padding_mask=None, feature_only=True)[0]`` of published BEATs (iter3 / iter3+ AS2M geometry).
Neither LAVIS nor BEATs' source is vendored in this project, so this is a plain ``torch.nn`` restatement of the published architecture
under BEATs' checkpoint key names:

* 16 x 16 patches of the ``[N, F, 128]`` filterbank (``F`` truncated to a multiple of 16) -> 512 channels, time-major token
  order ``p = t * 8 + f``; LayerNorm(512); ``post_extract_proj`` 512 -> 768;
* ``x + GELU(pos_conv(x))`` with a grouped, weight-normed ``Conv1d(768, 768, 128, padding=64, groups=16)`` (last output
  dropped), then ``encoder.layer_norm``;
* 12 post-LN layers with the deep-norm residual scale ``alpha = (2 * 12) ** 0.25`` and a T5-style bidirectional
  relative-position bias (320 buckets, max distance 800) that only layer 0 owns, scaled per (head, query) by a gate computed
  from the query's head slice.

The transformer is WavLM's encoder with two changes: ``alpha`` (WavLM: 1) and the gate's source (BEATs: the unscaled
q projection, WavLM: the layer input).  ``BEATsConfig(deep_norm_alpha=1.0, gate_from="input")`` is WavLM's encoder, and
``hf_state_dict`` / ``load_hf_state_dict`` map the transformer part onto ``transformers.WavLMEncoder``: that pins it
(``tests/test_beats.py``, ``tests/golden/beats.npz``).  The two deltas, the patch front end and the checkpoint key set are
restated from the published architecture and are not pinned to any running code.  Random weights only (no download).
"""
from __future__ import annotations

import logging
import math
from dataclasses import dataclass, fields
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from ._hip import HipEncoder


@dataclass
class BEATsConfig:
    """BEATs' configuration fields (the ``cfg`` dict of a checkpoint uses the same names; others are ignored)."""
    encoder_layers: int = 12
    encoder_embed_dim: int = 768
    encoder_ffn_embed_dim: int = 3072
    encoder_attention_heads: int = 12
    embed_dim: int = 512             # patch embedding width
    input_patch_size: int = 16
    mel_bins: int = 128
    conv_pos: int = 128
    conv_pos_groups: int = 16
    num_buckets: int = 320
    max_distance: int = 800
    layer_norm_eps: float = 1e-5
    deep_norm_alpha: Optional[float] = None   # None: BEATs' deep norm, (2 * encoder_layers) ** 0.25
    gate_from: str = "q"                      # "q": BEATs (unscaled q projection); "input": WavLM (layer input)

    def __post_init__(self):
        if self.deep_norm_alpha is None:
            self.deep_norm_alpha = float((2 * self.encoder_layers) ** 0.25)
        if self.gate_from not in ("q", "input"):
            raise ValueError("gate_from must be 'q' (BEATs) or 'input' (WavLM)")

    @classmethod
    def from_checkpoint_cfg(cls, cfg: dict) -> "BEATsConfig":
        names = {f.name for f in fields(cls)}
        kw = {k: v for k, v in cfg.items() if k in names}
        if "deep_norm_alpha" not in cfg and "deep_norm" in cfg and not cfg["deep_norm"]:
            kw["deep_norm_alpha"] = 1.0
        return cls(**kw)


def relative_position_bucket(rel: torch.Tensor, num_buckets: int = 320, max_distance: int = 800) -> torch.Tensor:
    """T5's bidirectional bucket of ``rel = key - query``, in the exact operation order of WavLM / BEATs (float32 log)."""
    nb = num_buckets // 2
    buckets = (rel > 0).to(torch.long) * nb
    rel = torch.abs(rel)
    max_exact = nb // 2
    is_small = rel < max_exact
    large = torch.log(rel.float() / max_exact)
    large = large / math.log(max_distance / max_exact)
    large = large * (nb - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return buckets + torch.where(is_small, rel, large)


class _WNConv1d(nn.Module):
    """Grouped Conv1d with weight norm over dims 0 and 1 (per tap): ``w = weight_g * weight_v / ||weight_v||``."""

    def __init__(self, dim: int, k: int, groups: int):
        super().__init__()
        self.k, self.groups = k, groups
        self.weight_g = nn.Parameter(torch.ones(1, 1, k))
        self.weight_v = nn.Parameter(torch.zeros(dim, dim // groups, k))
        self.bias = nn.Parameter(torch.zeros(dim))

    def effective_weight(self) -> torch.Tensor:
        v = self.weight_v
        return self.weight_g * v / v.norm(dim=(0, 1), keepdim=True)

    def forward(self, x):   # [N, C, P] -> [N, C, P + 1]
        return F.conv1d(x, self.effective_weight(), self.bias, padding=self.k // 2, groups=self.groups)


class _Attention(nn.Module):
    def __init__(self, cfg: BEATsConfig, has_bias_table: bool):
        super().__init__()
        d, h = cfg.encoder_embed_dim, cfg.encoder_attention_heads
        self.heads, self.hd, self.gate_from = h, d // h, cfg.gate_from
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (nn.Linear(d, d) for _ in range(4))
        self.grep_linear = nn.Linear(self.hd, 8)
        self.grep_a = nn.Parameter(torch.ones(1, h, 1, 1))
        if has_bias_table:
            self.relative_attention_bias = nn.Embedding(cfg.num_buckets, h)

    def forward(self, x, pos_bias):   # x [N, P, D], pos_bias [H, P, P]
        n, p, d = x.shape
        q, k, v = self.q_proj(x), self.k_proj(x), self.v_proj(x)
        src = q if self.gate_from == "q" else x
        u = self.grep_linear(src.view(n, p, self.heads, self.hd).transpose(1, 2)).view(n, self.heads, p, 2, 4).sum(-1)
        ga, gb = torch.sigmoid(u).chunk(2, dim=-1)
        gate = ga * (gb * self.grep_a - 1.0) + 2.0                      # [N, H, P, 1]
        heads = lambda t: t.view(n, p, self.heads, self.hd).transpose(1, 2)
        s = torch.matmul(heads(q) / math.sqrt(self.hd), heads(k).transpose(-1, -2)) + gate * pos_bias.to(x.dtype)
        o = torch.matmul(torch.softmax(s.float(), dim=-1).to(x.dtype), heads(v))
        return self.out_proj(o.transpose(1, 2).reshape(n, p, d))


class _Layer(nn.Module):
    def __init__(self, cfg: BEATsConfig, has_bias_table: bool):
        super().__init__()
        d, eps = cfg.encoder_embed_dim, cfg.layer_norm_eps
        self.alpha = cfg.deep_norm_alpha
        self.self_attn = _Attention(cfg, has_bias_table)
        self.self_attn_layer_norm = nn.LayerNorm(d, eps=eps)
        self.fc1 = nn.Linear(d, cfg.encoder_ffn_embed_dim)
        self.fc2 = nn.Linear(cfg.encoder_ffn_embed_dim, d)
        self.final_layer_norm = nn.LayerNorm(d, eps=eps)

    def forward(self, x, pos_bias):
        x = self.self_attn_layer_norm(self.alpha * x + self.self_attn(x, pos_bias))
        return self.final_layer_norm(self.alpha * x + self.fc2(F.gelu(self.fc1(x))))


class _Encoder(nn.Module):
    def __init__(self, cfg: BEATsConfig):
        super().__init__()
        self.cfg = cfg
        self.pos_conv = nn.ModuleList([_WNConv1d(cfg.encoder_embed_dim, cfg.conv_pos, cfg.conv_pos_groups)])
        self.layer_norm = nn.LayerNorm(cfg.encoder_embed_dim, eps=cfg.layer_norm_eps)
        self.layers = nn.ModuleList([_Layer(cfg, i == 0) for i in range(cfg.encoder_layers)])

    def position_bias(self, p: int) -> torch.Tensor:
        """``[H, P, P]``: ``E[bucket(j - i), h]`` from layer 0's table (every layer uses it)."""
        pos = torch.arange(p)
        b = relative_position_bucket(pos[None, :] - pos[:, None], self.cfg.num_buckets, self.cfg.max_distance)
        return self.layers[0].self_attn.relative_attention_bias(b.to(self.layers[0].self_attn.relative_attention_bias.weight.device)).permute(2, 0, 1)

    def forward(self, x):   # [N, P, D]
        p = x.shape[1]
        x = x + F.gelu(self.pos_conv[0](x.transpose(1, 2))[:, :, :p]).transpose(1, 2)
        x = self.layer_norm(x)
        pb = self.position_bias(p)
        for layer in self.layers:
            x = layer(x, pb)
        return x


class BEATs(nn.Module):
    """``model(fbank [N, F, 128]) -> [N, P, 768]`` with ``P = F // 16 * 8``; fp32 restatement (see the module docstring)."""

    def __init__(self, cfg: Optional[BEATsConfig] = None, **kw):
        super().__init__()
        cfg = cfg if cfg is not None else BEATsConfig(**kw)
        self.cfg = cfg
        self.num_features = cfg.encoder_embed_dim
        ps = cfg.input_patch_size
        self.patch_embedding = nn.Conv2d(1, cfg.embed_dim, kernel_size=ps, stride=ps, bias=False)
        self.layer_norm = nn.LayerNorm(cfg.embed_dim, eps=cfg.layer_norm_eps)
        self.post_extract_proj = nn.Linear(cfg.embed_dim, cfg.encoder_embed_dim)
        self.encoder = _Encoder(cfg)

    def tokens(self, frames: int) -> int:
        ps = self.cfg.input_patch_size
        return frames // ps * (self.cfg.mel_bins // ps)

    def front_end(self, fbank):
        """Patch embedding -> LayerNorm -> projection: ``[N, F, 128] -> [N, P, 768]`` (time-major tokens)."""
        ps = self.cfg.input_patch_size
        f = fbank.shape[1] // ps * ps
        x = self.patch_embedding(fbank[:, :f].unsqueeze(1).to(self.patch_embedding.weight.dtype))
        x = x.reshape(x.shape[0], x.shape[1], -1).transpose(1, 2)
        return self.post_extract_proj(self.layer_norm(x))

    def forward(self, fbank):
        return self.encoder(self.front_end(fbank))

    # ---- weights ---------------------------------------------------------------------------------------------
    @torch.no_grad()
    def init_seeded_(self, seed: int = 0) -> "BEATs":
        """Seeded synthetic weights (no BEATs checkpoint exists offline), drawn on the CPU in ``state_dict()`` order from one
        generator: matrices and biases N(0, 0.02), LayerNorm gains 1 + N(0, 0.1) and biases N(0, 0.05), ``grep_linear``
        N(0, 0.1) (so the gates spread), ``grep_a`` 1 + N(0, 0.3) per head, the bias table N(0, 0.5), the positional
        convolution's ``weight_g`` 2 + N(0, 0.2) per tap (its output is then of unit scale)."""
        g = torch.Generator().manual_seed(seed)
        for k, p in self.state_dict().items():
            r = torch.randn(p.shape, generator=g)
            if "layer_norm" in k:
                v = 1.0 + r * 0.1 if k.endswith("weight") else r * 0.05
            elif k.endswith("grep_a"):
                v = 1.0 + r * 0.3
            elif k.endswith("relative_attention_bias.weight"):
                v = r * 0.5
            elif k.endswith("weight_g"):
                v = 2.0 + r * 0.2
            elif "grep_linear" in k:
                v = r * 0.1
            else:
                v = r * 0.02
            p.copy_(v.to(p.dtype))
        return self

    _HF_LAYER = (("self_attn.q_proj", "attention.q_proj"), ("self_attn.k_proj", "attention.k_proj"),
                 ("self_attn.v_proj", "attention.v_proj"), ("self_attn.out_proj", "attention.out_proj"),
                 ("self_attn.grep_linear", "attention.gru_rel_pos_linear"), ("self_attn_layer_norm", "layer_norm"),
                 ("fc1", "feed_forward.intermediate_dense"), ("fc2", "feed_forward.output_dense"),
                 ("final_layer_norm", "final_layer_norm"))

    def _hf_names(self):
        """(this module's key, ``WavLMEncoder`` key) for every transformer parameter.  Name map::

            encoder.pos_conv.0.weight_g / weight_v / bias   pos_conv_embed.conv.parametrizations.weight.original0 / original1, conv.bias
            encoder.layer_norm                              layer_norm
            encoder.layers.i.self_attn.{q,k,v,out}_proj     layers.i.attention.{q,k,v,out}_proj
            encoder.layers.i.self_attn.grep_linear          layers.i.attention.gru_rel_pos_linear
            encoder.layers.i.self_attn.grep_a               layers.i.attention.gru_rel_pos_const
            encoder.layers.0.self_attn.relative_attention_bias   layers.0.attention.rel_attn_embed
            encoder.layers.i.self_attn_layer_norm           layers.i.layer_norm
            encoder.layers.i.fc1 / fc2                      layers.i.feed_forward.intermediate_dense / output_dense
            encoder.layers.i.final_layer_norm               layers.i.final_layer_norm
        """
        out = [("encoder.pos_conv.0.weight_g", "pos_conv_embed.conv.parametrizations.weight.original0"),
               ("encoder.pos_conv.0.weight_v", "pos_conv_embed.conv.parametrizations.weight.original1"),
               ("encoder.pos_conv.0.bias", "pos_conv_embed.conv.bias"),
               ("encoder.layer_norm.weight", "layer_norm.weight"), ("encoder.layer_norm.bias", "layer_norm.bias")]
        for i in range(len(self.encoder.layers)):
            for a, b in self._HF_LAYER:
                for s in ("weight", "bias"):
                    out.append((f"encoder.layers.{i}.{a}.{s}", f"layers.{i}.{b}.{s}"))
            out.append((f"encoder.layers.{i}.self_attn.grep_a", f"layers.{i}.attention.gru_rel_pos_const"))
        out.append(("encoder.layers.0.self_attn.relative_attention_bias.weight", "layers.0.attention.rel_attn_embed.weight"))
        return out

    def hf_state_dict(self) -> dict:
        """The transformer's weights under ``transformers.WavLMEncoder`` key names (see ``_hf_names``)."""
        sd = self.state_dict()
        return {b: sd[a].detach().clone() for a, b in self._hf_names()}

    @torch.no_grad()
    def load_hf_state_dict(self, sd: dict) -> None:
        """Inverse of ``hf_state_dict``: the transformer part from a ``WavLMEncoder`` state dict."""
        own = self.state_dict()
        for a, b in self._hf_names():
            own[a].copy_(sd[b])

    def hf_config(self):
        """The ``transformers.WavLMConfig`` of this geometry (its encoder is this module's transformer in WavLM mode)."""
        from transformers import WavLMConfig
        c = self.cfg
        return WavLMConfig(hidden_size=c.encoder_embed_dim, num_hidden_layers=c.encoder_layers, num_attention_heads=c.encoder_attention_heads,
                           intermediate_size=c.encoder_ffn_embed_dim, hidden_act="gelu", feat_extract_activation="gelu",
                           num_conv_pos_embeddings=c.conv_pos, num_conv_pos_embedding_groups=c.conv_pos_groups,
                           num_buckets=c.num_buckets, max_bucket_distance=c.max_distance, layer_norm_eps=c.layer_norm_eps,
                           hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, layerdrop=0.0, do_stable_layer_norm=False)

    def flops_per_chunk(self, frames: int) -> float:
        """Executed multiply-add flops x 2 of one ``[frames, 128]`` input (GEMMs, attention, positional convolution, patches)."""
        c = self.cfg
        p, d, i = self.tokens(frames), c.encoder_embed_dim, c.encoder_ffn_embed_dim
        layer = 2 * p * d * 3 * d + 4 * p * p * d + 2 * p * d * d + 4 * p * d * i
        front = 2 * p * c.input_patch_size ** 2 * c.embed_dim + 2 * p * c.embed_dim * d
        conv = 2 * p * d * (d // c.conv_pos_groups) * c.conv_pos
        return float(c.encoder_layers * layer + front + conv)


# keys a checkpoint may lack: BEATs' k_proj has no bias in some releases (treated as zero)
_OPTIONAL = (".self_attn.k_proj.bias",)


class HipBEATs(HipEncoder, BEATs):
    """The same encoder on the HIP extension (``mra_beats_*``, ``mraudio_amd/csrc/beats.hip``): this module is the parameter
    container (state_dict keys unchanged); ``forward`` runs ALL given chunks as one batched pass of hand-written gfx950 kernels
    -- f16 MFMA operands, fp32 accumulation, residual stream, LayerNorm statistics and softmax -- and returns fp32
    ``[n, P, 768]``.  The positional convolution's weight norm is folded into the effective weight when the weights are
    loaded (the encoder is frozen).  No CPU path."""

    _PREFIX = "mra_beats"   # options (``set_option``): ``"gemm_persist"`` 0 / 1

    def __init__(self, cfg: Optional[BEATsConfig] = None, device=None, **kw):
        super().__init__(cfg, **kw)
        import ctypes as C

        from .. import _lib
        c = self.cfg
        hc = _lib.mra_beats_cfg()
        _lib.lib().mra_beats_cfg_default(C.byref(hc))
        hc.dim, hc.heads, hc.ffn, hc.layers = c.encoder_embed_dim, c.encoder_attention_heads, c.encoder_ffn_embed_dim, c.encoder_layers
        hc.embed_dim, hc.patch, hc.mel_bins = c.embed_dim, c.input_patch_size, c.mel_bins
        hc.conv_pos, hc.conv_pos_groups, hc.num_buckets, hc.max_distance = c.conv_pos, c.conv_pos_groups, c.num_buckets, c.max_distance
        hc.ln_eps, hc.deep_norm_alpha = c.layer_norm_eps, float(c.deep_norm_alpha)
        hc.gate_from = _lib.MRA_BEATS_GATE_Q if c.gate_from == "q" else _lib.MRA_BEATS_GATE_INPUT
        self._create(hc, device)

    def _upload_tensors(self) -> dict:
        sd = dict(self.state_dict())
        del sd["encoder.pos_conv.0.weight_g"], sd["encoder.pos_conv.0.weight_v"]
        sd["encoder.pos_conv.0.weight"] = self.encoder.pos_conv[0].effective_weight().float()   # the weight norm, folded (frozen encoder)
        return sd

    @torch.no_grad()
    def forward(self, fbank):
        lib = self._lib
        self.sync_weights()
        x = fbank.to(self._device)
        if x.dtype not in (torch.float32, torch.float16):
            x = x.float()
        x = x.contiguous()
        n, frames = int(x.shape[0]), int(x.shape[1])
        if x.dim() != 3 or int(x.shape[2]) != self.cfg.mel_bins:
            raise ValueError(f"fbank must be [N, F, {self.cfg.mel_bins}], got {list(x.shape)}")
        out = torch.empty(n, self.tokens(frames), self.num_features, dtype=torch.float32, device=self._device)
        if n == 0:
            return out
        with torch.cuda.device(self._device):
            nbytes = int(lib.lib().mra_beats_workspace_bytes(self._handle, n, frames))
            if nbytes == 0:
                lib.check(-1, "mra_beats_workspace_bytes")
            ws = self._workspace(nbytes)
            self._call("forward", lib.ptr(x), lib.mra_dtype(x.dtype), n, frames, lib.ptr(out), lib.ptr(ws), ws.numel(), lib.current_stream())
        return out

    def flops(self, n: int, frames: int) -> float:
        return float(self._lib.lib().mra_beats_flops(self._handle, n, frames))


def load_beats_checkpoint(model: BEATs, state: dict) -> None:
    """Loads a BEATs ``state_dict`` (the ``"model"`` entry of a checkpoint) into ``model``.  Keys the model does not have
    (``predictor.*`` of fine-tuned checkpoints, ...) are ignored; an absent ``k_proj.bias`` is taken as zero; any other
    missing key raises ``KeyError`` naming it."""
    own = model.state_dict()
    missing = [k for k in own if k not in state and not k.endswith(_OPTIONAL)]
    if missing:
        raise KeyError(f"BEATs checkpoint lacks {len(missing)} required key(s): {', '.join(missing[:8])}" + (" ..." if len(missing) > 8 else ""))
    with torch.no_grad():
        for k, p in own.items():
            if k in state:
                t = state[k]
                if tuple(t.shape) != tuple(p.shape):
                    raise ValueError(f"BEATs checkpoint key {k}: shape {tuple(t.shape)}, expected {tuple(p.shape)}")
                p.copy_(t.to(p.dtype))
            else:
                p.zero_()
    if isinstance(model, HipBEATs):
        model._dirty = True


class BeatsEncoder(nn.Module):
    """The reference's callee (LAVIS ``BeatsEncoder(checkpoint_path)``): ``forward(fbank [N, F, 128]) -> [N, P, 768]``,
    ``num_features = 768``.  ``checkpoint_path`` is a BEATs checkpoint ``{"cfg": {...}, "model": state_dict}``; without one the
    encoder keeps the seeded synthetic init (and says so).  ``backend="hip"`` runs it on this build's kernels (the default),
    ``"torch"`` is the fp32 restatement."""

    def __init__(self, checkpoint_path: Optional[str] = None, backend: str = "hip", device=None, seed: int = 0):
        super().__init__()
        if backend not in ("hip", "torch"):
            raise ValueError("backend must be 'hip' or 'torch'")
        ckpt = None
        cfg = BEATsConfig()
        if checkpoint_path is not None:
            ckpt = checkpoint_path if isinstance(checkpoint_path, dict) else torch.load(checkpoint_path, map_location="cpu", weights_only=False)
            if not isinstance(ckpt, dict) or "model" not in ckpt:
                raise ValueError("a BEATs checkpoint is a dict {'cfg': {...}, 'model': state_dict}")
            cfg = BEATsConfig.from_checkpoint_cfg(dict(ckpt.get("cfg") or {}))
        self.model = HipBEATs(cfg, device=device) if backend == "hip" else BEATs(cfg)
        self.num_features = self.model.num_features
        if ckpt is None:
            self.model.init_seeded_(seed)
            logging.warning("BeatsEncoder: no checkpoint_path was given, the audio encoder has SYNTHETIC seeded weights (seed %d) -- "
                            "its features are not meaningful.", seed)
            self.weights_source = f"synthetic (seed {seed})"
        else:
            load_beats_checkpoint(self.model, ckpt["model"])
            self.weights_source = str(checkpoint_path) if not isinstance(checkpoint_path, dict) else "checkpoint dict"
        if backend == "torch" and device is not None:
            self.model.to(device)

    @torch.no_grad()
    def forward(self, fbank):
        return self.model(fbank)
