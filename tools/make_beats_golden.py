"""Golden vectors for the BEATs restatement (row A1 / N4, the audio half).

Source of truth for the transformer: ``transformers.WavLMEncoder`` (HF modeling_wavlm.py: post-LN layers, grouped weight-normed
positional convolution, T5-style bidirectional relative-position buckets owned by layer 0, the gated bias) -- BEATs' transformer
is that encoder with the deep-norm residual scale and the gate taken from the q projection; in WavLM mode (``deep_norm_alpha = 1``,
``gate_from = "input"``) the restatement IS it.  Full width (768, 12 heads, FFN 3072), LAYERS layers.  The patch front end in front
of it (``BEATs.front_end``: 16 x 16 patches -> LayerNorm(512) -> 512 -> 768) is the restatement's own: no running code of it exists
offline.  Weights are NOT stored: they are re-derived from the seed by ``BEATs.init_seeded_`` and mapped into the HF encoder by
``hf_state_dict``; the filterbanks come from ``make_fbank``.  Stored per case (512 frames -> 256 tokens, 1000 frames -> 496 tokens):
the HF encoder's output at a few token rows plus per-token checksums of every token.

    python tools/make_beats_golden.py        # writes tests/golden/beats.npz
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS, WEIGHT_SEED, INPUT_SEED, CHUNKS = 2, 21, 22, 2
CASES = {"s256": 512, "s496": 1000}        # name -> frames
ROWS = {"s256": [0, 1, 7, 8, 128, 255], "s496": [0, 9, 247, 248, 400, 495]}


def make_fbank(frames: int, n: int = CHUNKS, seed: int = INPUT_SEED) -> torch.Tensor:
    """Seeded normalised filterbanks [n, frames, 128] fp32 (shared by the generator and the tests)."""
    return torch.randn(n, frames, 128, generator=torch.Generator().manual_seed(seed + frames))


def wavlm_model():
    from mraudio_amd.models.beats import BEATs, BEATsConfig
    return BEATs(BEATsConfig(encoder_layers=LAYERS, deep_norm_alpha=1.0, gate_from="input")).eval().init_seeded_(WEIGHT_SEED)


def hf_reference(model, fbank):
    """The restated front end, then ``transformers.WavLMEncoder`` on the mapped weights."""
    from transformers.models.wavlm.modeling_wavlm import WavLMEncoder
    hf = WavLMEncoder(model.hf_config()).eval()
    hf.load_state_dict(model.hf_state_dict(), strict=True)
    with torch.no_grad():
        return hf(model.front_end(fbank)).last_hidden_state


def golden_arrays(model=None) -> dict:
    model = model if model is not None else wavlm_model()
    out = {}
    for name, frames in CASES.items():
        ref = hf_reference(model, make_fbank(frames))
        out[f"{name}_rows"] = ref[:, ROWS[name]].numpy().astype(np.float32)
        out[f"{name}_token_sum"] = ref.sum(-1).numpy().astype(np.float32)
        out[f"{name}_token_sq_sum"] = ref.pow(2).sum(-1).numpy().astype(np.float32)
    out["meta"] = np.array(json.dumps(dict(layers=LAYERS, weight_seed=WEIGHT_SEED, input_seed=INPUT_SEED, chunks=CHUNKS, cases=CASES, rows=ROWS,
                                           mode="WavLM (deep_norm_alpha 1, gate from the layer input)",
                                           source="restated BEATs front end + transformers WavLMEncoder, last_hidden_state")))
    return out


if __name__ == "__main__":
    torch.set_num_threads(8)
    arrays = golden_arrays()
    path = os.path.join(ROOT, "tests", "golden", "beats.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, {k: v.shape for k, v in arrays.items()})
