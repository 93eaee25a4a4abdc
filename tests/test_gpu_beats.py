"""``-m gpu``: row A1 / N4, the audio half -- the BEATs encoder on the HIP extension (``mra_beats_*``, ``csrc/beats.hip``) against the
committed WavLM vectors (``tests/golden/beats.npz``: transformers ``WavLMEncoder`` behind the restated front end) and against the fp32
torch restatement (``mraudio_amd/models/beats.py``) in BEATs mode at full depth; then through ``XInstructBLIP(audio_encoder="beats")``.

Tolerance: MFMA operands are f16 (the reference autocasts the encoders to fp16); accumulation, residual stream, LayerNorm statistics
and softmax fp32.  The bars were set before any measurement: WavLM mode |d| <= 2e-2 and relative Frobenius <= 2e-3; BEATs mode,
12 layers, |d| <= 3e-2 and relative Frobenius <= 3e-3 (post-LN keeps activations near unit scale)."""
import json
import os

import numpy as np
import pytest
import torch

from mraudio_amd.models.beats import BEATs, BEATsConfig, BeatsEncoder, HipBEATs
from tools.make_beats_golden import CASES, LAYERS, ROWS, make_fbank, wavlm_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


def _hip_like(ref, dev):
    hip = HipBEATs(ref.cfg, device=dev).eval()
    hip.load_state_dict(ref.state_dict())
    return hip


def test_hip_wavlm_mode_matches_the_hf_vectors(golden_dir, dev):
    gold = np.load(os.path.join(golden_dir, "beats.npz"))
    assert json.loads(str(gold["meta"]))["layers"] == LAYERS
    hip = _hip_like(wavlm_model(), dev)
    for name, frames in CASES.items():
        y = hip(make_fbank(frames).to(dev)).cpu()
        assert y.shape == (2, frames // 16 * 8, 768) and y.dtype == torch.float32 and torch.isfinite(y).all()
        rows = y[:, ROWS[name]].numpy()
        want = gold[f"{name}_rows"]
        d = np.abs(rows - want).max()
        rel = float(np.linalg.norm(rows - want) / np.linalg.norm(want))
        print(f"beats WavLM mode {name}: max|d| {d:.3e}, rel {rel:.3e}")
        assert d <= 2e-2 and rel <= 2e-3, (name, d, rel)
        assert np.abs(y.sum(-1).numpy() - gold[f"{name}_token_sum"]).max() < 0.5


@pytest.fixture(scope="module")
def beats12(dev):
    ref = BEATs().eval().init_seeded_(31)
    return ref, _hip_like(ref, dev)


@pytest.mark.parametrize("frames", [512, 992])
def test_hip_beats_mode_12_layers_against_the_fp32_restatement(beats12, dev, frames):
    ref, hip = beats12
    fb = make_fbank(frames, n=2, seed=40)
    with torch.no_grad():
        want = ref(fb)
    y = hip(fb.to(dev)).cpu()
    d, rel = (y - want).abs().max().item(), _rel(y, want)
    print(f"beats 12 layers, {frames} frames (S = {want.shape[1]}): max|d| {d:.3e}, rel {rel:.3e}")
    assert torch.isfinite(y).all() and d <= 3e-2 and rel <= 3e-3, (d, rel)


@pytest.mark.parametrize("frames", [512, 992])
def test_hip_in_kernel_bias_and_gate_drive_the_output(dev, frames):
    """The bias table scaled up until attention rows peak: the gated relative-position bias dominates the scores, so a kernel that
    dropped or mis-indexed it (or its gate) could not meet the same bars."""
    ref = BEATs().eval().init_seeded_(32)
    with torch.no_grad():
        ref.encoder.layers[0].self_attn.relative_attention_bias.weight.mul_(20.0)
    fb = make_fbank(frames, n=2, seed=41)
    with torch.no_grad():
        p = ref.encoder.position_bias(ref.tokens(frames))
        peak = torch.softmax(p, -1).max(-1).values.mean().item()          # typical row maximum of the bias alone
        want = ref(fb)
        flat = BEATs().eval().init_seeded_(32)(fb)
    assert peak > 0.4, peak
    assert (want - flat).abs().max().item() > 0.5                         # the bias moves the output far beyond the bars
    y = _hip_like(ref, dev)(fb.to(dev)).cpu()
    d, rel = (y - want).abs().max().item(), _rel(y, want)
    print(f"beats peaked bias, {frames} frames: mean row peak {peak:.2f}, max|d| {d:.3e}, rel {rel:.3e}")
    assert torch.isfinite(y).all() and d <= 3e-2 and rel <= 3e-3, (d, rel)


def test_hip_chunks_are_independent_and_f16_input_is_accepted(beats12, dev):
    ref, hip = beats12
    fb = make_fbank(512, n=3, seed=42).to(dev)
    y = hip(fb)
    more = torch.cat([make_fbank(512, n=5, seed=43).to(dev), fb])
    ym = hip(more)
    assert (ym[5:] - y).abs().max().item() <= 1e-4
    assert (hip(fb[1:2]) - y[1:2]).abs().max().item() <= 1e-4
    y16 = hip(fb.half()).cpu()
    with torch.no_grad():
        want = ref(fb.half().float().cpu())
    assert (y16 - want).abs().max().item() <= 3e-2 and _rel(y16, want) <= 3e-3
    # F not a multiple of 16: truncated, as the restatement does
    odd = make_fbank(519, n=1, seed=44)
    with torch.no_grad():
        wo = ref(odd)
    yo = hip(odd.to(dev)).cpu()
    assert yo.shape == wo.shape == (1, 256, 768) and (yo - wo).abs().max().item() <= 3e-2


def test_hip_beats_errors(dev):
    from mraudio_amd import MraError

    fresh = HipBEATs(BEATsConfig(encoder_layers=1), device=dev)
    fresh._dirty, fresh._ver = False, sum(p._version for p in fresh.parameters())   # nothing uploaded: the library must refuse to run
    with pytest.raises(MraError):
        fresh(make_fbank(512, n=1).to(dev))
    hip = _hip_like(BEATs(BEATsConfig(encoder_layers=1)).init_seeded_(1), dev)
    # (the refusal of 1040 frames = 520 tokens sits next to the 1024-frame pass: tests/test_gpu_encoder_cores.py)
    assert hip(torch.zeros(0, 512, 128, device=dev)).shape == (0, 256, 768)


def test_raw_fbank_through_the_model_uses_the_hip_encoder(dev):
    """samples["audio"] [B, T, 512, 128] -> one [B * T] batch through BeatsEncoder on the HIP kernels -> audio_ln -> Q-Former -> scores:
    equal to feeding the fp32 restatement's features as ``audio_embeds`` (reference :267-306), within the headline logit bar."""
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    model = XInstructBLIP(seed=0, perturb=True, device=dev, modalities=["audio"], audio_encoder="beats")
    assert isinstance(model.audio_encoder, BeatsEncoder) and isinstance(model.audio_encoder.model, HipBEATs)
    ref = BEATs().eval().init_seeded_(0)                 # BeatsEncoder without a checkpoint keeps the seed-0 init
    B, T = 2, 3
    audio = torch.randn(B, T, 512, 128, generator=torch.Generator().manual_seed(9))
    prompts = ["Query: a dog barks.\nRelevant windows: ", "Query: music starts.\nRelevant windows: "]
    base = {"text_input": prompts, "timestamps": [[0, 2, 4], [1, 3, 5]], "duration": [6, 6]}
    model.encode_chunk = 4                               # 6 chunks -> 4 + 2
    out = model.encode_fuse({**base, "audio": audio})
    with torch.no_grad():
        feats = torch.stack([ref(audio[b]) for b in range(B)])
    want = model.encode_fuse({**base, "audio_embeds": feats})
    dl = (out["fused"] - want["fused"]).abs().max().item()
    print(f"beats through XInstructBLIP: max|d fused logit| {dl:.3e}")
    assert dl <= 1e-3
