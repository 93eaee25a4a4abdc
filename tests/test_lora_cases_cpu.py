"""The LoRA branch without a GPU: the references, bounds, emulations and mutants of tests/lora_cases.py agree with each other, the
counter-based dropout behaves like a Bernoulli mask, the three ABI entries refuse bad arguments before any launch, and the Python side
(``LoraLinear``, ``apply_lora``, the state-dict keys, the model's checkpoint routing, the trainer, the CLI) does what it says on the CPU
path -- the path that is the oracle of tests/test_gpu_lora.py."""
import ctypes as C
import math
import os

import pytest
import torch
from torch import nn

import lora_cases as LC
from mraudio_amd import _lib
from mraudio_amd.models import lora as L


def _id(dt):
    return "f16" if dt == torch.float16 else "bf16"


SMALL = [(m, w, r, p) for (m, w, r, p) in LC.cases() if r in (5, 16) and w in (8, 40, 264) and p in (0.0, 0.5)]


# ---- emulations inside, mutants outside ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", LC.DTYPES, ids=_id)
def test_emulations_sit_inside_their_bounds(dtype):
    worst = {"down": 0.0, "up": 0.0, "wgrad": 0.0}
    for rows, width, R, p in SMALL:
        c = LC.make_case(rows, width, R, dtype)
        keep, iq = LC.mask(rows, width, p), LC.inv_q(p)
        for layout in (LC.NR, LC.RN):
            ref, b = LC.down_ref(c["x"], c["W"], iq, keep)
            worst["down"] = max(worst["down"], LC.ratio(LC.down_emulate(c["x"], c["W"], layout, iq, p), ref, b))
            ref, b = LC.up_ref(c["y0"], c["u"], c["W"], iq, keep)
            worst["up"] = max(worst["up"], LC.ratio(LC.up_emulate(c["y0"], c["u"], c["W"], layout, iq, p).float(), ref, b))
            ref, b = LC.wgrad_ref(c["x"], c["u"], c["dW0"], iq, keep)
            worst["wgrad"] = max(worst["wgrad"], LC.ratio(LC.wgrad_emulate(c["x"], c["u"], c["dW0"], layout, iq, p), ref, b))
    print(f"lora emulations {_id(dtype)}: worst ratio to bound {worst}")
    assert all(0.0 < v <= 1.0 for v in worst.values()), worst          # fp32 emulations do not reproduce float64


def _outside(kind, mutant, dtype):
    out = []
    for rows, width, R, p in SMALL:
        c = LC.make_case(rows, width, R, dtype)
        ld, keep, iq = width + 8, LC.mask(rows, width, p), LC.inv_q(p)
        for layout in (LC.NR, LC.RN):
            if kind == "down":
                ref, b = LC.down_ref(c["x"], c["W"], iq, keep)
                got = LC.down_emulate(c["x"], c["W"], layout, iq, p, ld=ld, mutant=mutant)
            elif kind == "up":
                ref, b = LC.up_ref(c["y0"], c["u"], c["W"], iq, keep)
                got = LC.up_emulate(c["y0"], c["u"], c["W"], layout, iq, p, ld=ld, mutant=mutant).float()
            else:
                ref, b = LC.wgrad_ref(c["x"], c["u"], c["dW0"], iq, keep)
                got = LC.wgrad_emulate(c["x"], c["u"], c["dW0"], layout, iq, p, ld=ld, mutant=mutant)
            if LC.ratio(got, ref, b) > 1.0:
                out.append((rows, width, R, p))
    return set(out)


@pytest.mark.parametrize("dtype", LC.DTYPES, ids=_id)
@pytest.mark.parametrize("kind,mutant", [("down", m) for m in LC.DOWN_MUTANTS] + [("up", m) for m in LC.UP_MUTANTS]
                         + [("wgrad", m) for m in LC.WGRAD_MUTANTS])
def test_mutants_land_outside_somewhere(kind, mutant, dtype):
    outside = _outside(kind, mutant, dtype)
    assert outside, (kind, mutant)
    tile = {"down": 16, "up": 64, "wgrad": 32}[kind]
    if mutant == "tail_rows":                     # exactly the cases with a short last tile
        assert outside == {c for c in SMALL if c[0] % tile}
    if mutant in ("last_k_step_dropped", "prefill_overwritten", "u_unrounded"):
        assert outside == set(SMALL)
    if mutant == "scale_twice":                   # needs dropout: 1/q = 1 at p = 0
        assert outside == {c for c in SMALL if c[3] > 0}
    if mutant == "mask_ld":                       # ... and a second row: row 0 starts at index 0 under either pitch
        assert outside == {c for c in SMALL if c[3] > 0 and c[0] > 1}


# ---- keep ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.05, 0.5])
def test_keep_share_and_seed_independence(p):
    n = 1 << 20
    q = 1.0 - p
    sigma = math.sqrt(p * q / n)
    a = L.keep_mask(LC.SEED, 1024, 1024, p)
    b = L.keep_mask(LC.SEED + 1, 1024, 1024, p)
    for m in (a, b):
        assert abs(m.float().mean().item() - q) <= 4 * sigma
    # two seeds: the joint keep share is q^2 within 4 sigma of a Bernoulli(q^2) mean
    both = (a & b).float().mean().item()
    assert abs(both - q * q) <= 4 * math.sqrt(q * q * (1 - q * q) / n), both
    assert torch.equal(a, L.keep_mask(LC.SEED, 1024, 1024, p))            # a pure function of (seed, index)


def test_keep_edge_cases():
    assert L.keep_mask(7, 5, 8, 0.0).all()
    assert L.keep_threshold(0.0) == 0 and L.keep_threshold(0.5) == 1 << 31 and L.keep_threshold(1.0 - 2.0 ** -40) == 0xFFFFFFFF
    # the hash by hand for one index beyond 2^32 (hi32 enters through the golden-ratio multiply)
    idx, seed = (3 << 32) + 11, (5 << 32) + 9
    h = (11 ^ 9 ^ ((3 * 0x9E3779B9) & 0xFFFFFFFF) ^ 5) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> 16
    assert int(L.keep_hash(torch.tensor([idx], dtype=torch.int64), seed)) == h


# ---- the ABI entries without a device ------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf = C.create_string_buffer(1 << 14)
    p = (C.addressof(buf) + 15) // 16 * 16
    NR, RN, BF = _lib.MRA_LORA_NR, _lib.MRA_LORA_RN, _lib.MRA_BF16

    def down(x=p, ld=32, rows=4, K=32, dt=BF, w=p, R=8, lay=RN, scale=1.0, pr=0.0, out=p):
        return lib.mra_lora_down(x, ld, rows, K, dt, w, R, lay, scale, pr, 1, out, None)

    def up(y=p, ld=32, rows=4, N=32, dt=BF, u=p, R=8, w=p, lay=NR, scale=1.0, pr=0.0):
        return lib.mra_lora_up_add(y, ld, rows, N, dt, u, R, w, lay, scale, pr, 1, None)

    def wg(x=p, ld=32, rows=4, N=32, dt=BF, u=p, R=8, dw=p, lay=NR, scale=1.0, pr=0.0):
        return lib.mra_lora_wgrad(x, ld, rows, N, dt, u, R, dw, lay, scale, pr, 1, None)

    bad = [("null", dict(x=None)), ("null", dict(w=None)), ("R must", dict(R=0)), ("R must", dict(R=17)), ("multiple of 8", dict(K=36, ld=40)),
           ("ld < width", dict(ld=24)), ("pitch", dict(ld=36)), ("aligned", dict(x=p + 8)), ("aligned", dict(w=p + 4)), ("p must", dict(pr=1.0)),
           ("p must", dict(pr=-0.1)), ("dtype", dict(dt=_lib.MRA_F32)), ("layout", dict(lay=2)), ("negative rows", dict(rows=-1))]
    for fn, ren in ((down, {}), (up, {"x": "y", "K": "N", "w": "u"}), (wg, {"x": "x", "K": "N", "w": "dw"})):
        for msg, kw in bad:
            kw = {ren.get(k, k): v for k, v in kw.items()}
            assert fn(**kw) == -1, (fn.__name__, kw)
            assert msg.encode() in lib.mra_last_error(), (fn.__name__, kw, lib.mra_last_error())
        assert fn(rows=0) == 0                       # a no-op, no device needed
    assert down(out=None) == -1 and up(w=None) == -1 and wg(u=None) == -1


# ---- LoraLinear on the CPU -------------------------------------------------------------------------------------------------------------------
def test_lora_linear_cpu_matches_the_hand_written_formula_under_autograd():
    torch.manual_seed(3)
    base = nn.Linear(24, 40, dtype=torch.float64)
    mod = L.LoraLinear(base, r=5, alpha=10, dropout=0.5)
    A, B = mod.lora_A["default"].weight, mod.lora_B["default"].weight
    assert A.shape == (5, 24) and B.shape == (40, 5) and A.dtype == torch.float64 and not base.weight.requires_grad
    assert torch.count_nonzero(B) == 0 and A.abs().max() <= 1.0 / math.sqrt(24) + 1e-12            # kaiming-uniform, a = sqrt(5): bound 1 / sqrt(fan_in)
    assert {n for n, _ in mod.named_parameters()} == {"base_layer.weight", "base_layer.bias", "lora_A.default.weight", "lora_B.default.weight"}
    with torch.no_grad():
        B.copy_(torch.randn(40, 5, dtype=torch.float64))
    x = torch.randn(3, 7, 24, dtype=torch.float64, requires_grad=True)
    G = torch.randn(3, 7, 40, dtype=torch.float64)
    mod.train()
    torch.manual_seed(11)
    y = mod(x)
    (y * G).sum().backward()
    got = (y.detach(), x.grad.clone(), A.grad.clone(), B.grad.clone())
    keep = L.keep_mask(mod.last_seed, 21, 24, 0.5).reshape(3, 7, 24).double()
    assert 0 < keep.sum() < keep.numel()
    x2, A2, B2 = x.detach().clone().requires_grad_(True), A.detach().clone().requires_grad_(True), B.detach().clone().requires_grad_(True)
    y2 = nn.functional.linear(x2, base.weight, base.bias) + 2.0 * ((x2 * keep / 0.5) @ A2.t()) @ B2.t()
    (y2 * G).sum().backward()
    for a, b in zip(got, (y2.detach(), x2.grad, A2.grad, B2.grad)):
        assert (a - b).abs().max() <= 1e-12 * max(1.0, b.abs().max().item())
    # the same seed gives the same mask (activation checkpointing restores the CPU generator); eval mode drops nothing and draws nothing
    torch.manual_seed(11)
    assert torch.equal(mod(x), y)
    mod.eval()
    state = torch.get_rng_state()
    ye = mod(x)
    assert torch.equal(torch.get_rng_state(), state)
    ref = nn.functional.linear(x, base.weight, base.bias) + 2.0 * (x @ A.t()) @ B.t()
    assert (ye - ref).abs().max() <= 1e-12
    # grad_unscale multiplies the adapter gradients only
    mod.grad_unscale = 0.25
    A.grad = B.grad = x.grad = None
    (mod(x) * G).sum().backward()
    gA, gB, gx = A.grad.clone(), B.grad.clone(), x.grad.clone()
    mod.grad_unscale = 1.0
    A.grad = B.grad = x.grad = None
    (mod(x) * G).sum().backward()
    assert torch.allclose(gA * 4, A.grad, rtol=1e-12) and torch.allclose(gB * 4, B.grad, rtol=1e-12) and torch.allclose(gx, x.grad, rtol=1e-12)
    with pytest.raises(_lib.MraError, match="GPU"):
        L.LoraLinear(nn.Linear(8, 8), hip=True)(torch.randn(2, 8))


def _tiny_llama(dtype=torch.float32):
    tf = pytest.importorskip("transformers")
    torch.manual_seed(0)
    cfg = tf.LlamaConfig(vocab_size=64, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                         max_position_embeddings=64, pad_token_id=0, bos_token_id=2, eos_token_id=2)
    return tf.LlamaForCausalLM(cfg).to(dtype).eval().requires_grad_(False)


def test_apply_lora_on_a_tiny_llama_and_key_round_trip():
    llm = _tiny_llama()
    ids = torch.randint(3, 64, (2, 9), generator=torch.Generator().manual_seed(1))
    before = llm(input_ids=ids).logits
    names = L.apply_lora(llm, r=8, alpha=8, dropout=0.05)
    assert len(names) == 14 and not any("lm_head" in n for n in names) and isinstance(llm.lm_head, nn.Linear)
    assert {n.split(".")[-1] for n in names} == {"q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"}
    assert L.apply_lora(llm) == []                                         # already adapted: nothing new, nothing wrapped twice
    assert torch.equal(llm(input_ids=ids).logits, before)                  # B = 0: the same bits
    params = L.lora_parameters(llm)
    assert len(params) == 28 and all(p.requires_grad and p.dtype == torch.float32 for p in params)
    assert {id(p) for p in llm.parameters() if p.requires_grad} == {id(p) for p in params}
    sd = L.lora_state_dict(llm)
    assert len(sd) == 28 and "base_model.model.model.layers.1.self_attn.q_proj.lora_B.default.weight" in sd
    assert "model.layers.0.mlp.down_proj.base_layer.weight" in llm.state_dict()
    new = {k: torch.randn_like(v) for k, v in sd.items()}
    assert L.load_lora_state_dict(llm, new) == ([], [])
    assert all(torch.equal(v, new[k]) for k, v in L.lora_state_dict(llm).items())
    assert not torch.equal(llm(input_ids=ids).logits, before)
    first = next(iter(new))
    miss, unexp = L.load_lora_state_dict(llm, {"base_model.model.nowhere.lora_A.default.weight": new[first]})
    assert len(miss) == 28 and unexp == ["base_model.model.nowhere.lora_A.default.weight"]
    only_q = L.apply_lora(_tiny_llama(), target_modules=["q_proj"])
    assert len(only_q) == 2


# ---- the model's checkpoint routing, on a stand-in (the model itself needs a GPU) ------------------------------------------------------------
class _Stub(nn.Module):
    """What ``XInstructBLIP.load_state_dict`` / ``enable_lora`` touch, without Q-Formers."""
    from mraudio_amd.models.xinstructblip import XInstructBLIP as _X

    modalities, lora = [], False
    load_state_dict, enable_lora, lora_parameters, train = _X.load_state_dict, _X.enable_lora, _X.lora_parameters, _X.train

    def __init__(self, llm):
        super().__init__()
        object.__setattr__(self, "llm_model", llm)


def test_model_routes_ignores_and_reports_llm_model_keys():
    stub = _Stub(_tiny_llama())
    assert L.lora_state_dict(stub.llm_model) == {}                         # no adapters yet
    donor = _tiny_llama()
    L.apply_lora(donor)
    file = {f"llm_model.{k}": torch.full_like(v, 0.5) for k, v in L.lora_state_dict(donor).items()}
    msg = stub.load_state_dict(file, strict=True)                          # LoRA off: ignored exactly as before
    assert msg.missing_keys == [] and msg.unexpected_keys == []
    with pytest.raises(_lib.MraError, match="no LLM attached"):
        _Stub(None).enable_lora()
    stub.enable_lora(r=8, alpha=8, dropout=0.05)
    stub.enable_lora()                                                     # idempotent
    assert stub.lora and len(stub.lora_parameters()) == 28 and not any(k.startswith("llm_model") for k in stub.state_dict())
    msg = stub.load_state_dict(file, strict=True)
    assert msg.missing_keys == [] and msg.unexpected_keys == []
    assert all((p == 0.5).all() for p in stub.lora_parameters())
    part = dict(list(file.items())[:2])
    msg = stub.load_state_dict(part, strict=True)                          # missing adapter keys are reported, not raised on (reference :813-815)
    assert len(msg.missing_keys) == 26 and all(k.startswith("llm_model.base_model.model.") for k in msg.missing_keys)
    with pytest.raises(RuntimeError, match="unexpected"):
        stub.load_state_dict({"llm_model.base_model.model.nowhere.lora_A.default.weight": torch.zeros(1)}, strict=True)
    stub.train()
    assert all(m.training for m in stub._lora_mods) and not stub.llm_model.training
    stub.eval()
    assert not any(m.training for m in stub._lora_mods)


class _FileStub(_Stub):
    """One modality with stand-ins for its Q-Former, query tokens, LayerNorm and projection: the loader's strictness has something to miss."""
    from mraudio_amd.models.xinstructblip import XInstructBLIP as _X

    modalities = ["video"]
    _load_file, load_checkpoint, load_from_pretrained = _X._load_file, _X.load_checkpoint, _X.load_from_pretrained
    tokenizer, weights_source = None, "synthetic (seed 0)"

    def __init__(self, llm):
        super().__init__(llm)
        torch.manual_seed(2)
        self.video_Qformer, self.video_ln, self.video_llm_proj = nn.Linear(4, 4), nn.LayerNorm(4), nn.Linear(4, 4)
        self.video_query_tokens = nn.Parameter(torch.zeros(1, 2, 4))


def test_adapter_only_checkpoint_loads_with_default_flags(tmp_path):
    """What ``finetune --lora --freeze-qformers`` (and the reference's trainer) writes holds only ``llm_model.*`` keys.  ``load_checkpoint``
    with its default strictness takes it when LoRA is on and leaves the Q-Former side alone; with LoRA off such a file still raises; a file
    that does hold Q-Former keys is as strict as ever."""
    donor = _tiny_llama()
    L.apply_lora(donor)
    adapters = {f"llm_model.{k}": torch.full_like(v, 0.25) for k, v in L.lora_state_dict(donor).items()}
    path = str(tmp_path / "adapters.pth")
    torch.save({"model": adapters, "optimizer": {}, "scaler": None, "epoch": 0}, path)      # the trainer's file layout
    stub = _FileStub(_tiny_llama())
    with pytest.raises(RuntimeError, match="no key of this model's modalities"):            # LoRA off: as before
        stub.load_checkpoint(path)
    stub.enable_lora()
    before = {k: v.clone() for k, v in stub.state_dict().items()}
    msg = stub.load_checkpoint(path)                                                        # strict by default
    assert msg.missing_keys == [] and msg.unexpected_keys == []
    assert all((p == 0.25).all() for p in stub.lora_parameters())
    assert all(torch.equal(v, before[k]) for k, v in stub.state_dict().items())             # the Q-Former side is untouched
    assert stub.weights_source == f"synthetic (seed 0) + LoRA adapters of {path}"
    # a file that speaks about the Q-Former side is held to all of it
    mixed = dict(adapters, **{"video_ln.weight": torch.ones(4)})
    torch.save(mixed, path)
    with pytest.raises(RuntimeError, match="missing"):
        stub.load_checkpoint(path)
    msg = stub.load_from_pretrained(path)
    assert "video_query_tokens" in msg.missing_keys and "video_Qformer.weight" in msg.missing_keys
    full = dict(adapters, **{k: v for k, v in before.items()})
    torch.save(full, path)
    msg = stub.load_checkpoint(path)
    assert msg.missing_keys == [] and stub.weights_source == f"checkpoint {path}"


def test_automatic_route_falls_back_instead_of_raising():
    """``hip=None`` picks the HIP entries only for what they take; r > 16, an odd width or a dtype mismatch run as torch ops (here: on the
    CPU the choice is torch ops anyway, so the decision function is asked directly with a stand-in for a GPU tensor)."""
    class FakeCuda:
        is_cuda, dtype = True, torch.bfloat16

    ok = L.LoraLinear(nn.Linear(16, 24).to(torch.bfloat16), r=8)
    assert ok._use_hip(FakeCuda()) is True
    for mod in (L.LoraLinear(nn.Linear(16, 24).to(torch.bfloat16), r=17), L.LoraLinear(nn.Linear(12, 24).to(torch.bfloat16), r=8),
                L.LoraLinear(nn.Linear(16, 20).to(torch.bfloat16), r=8), L.LoraLinear(nn.Linear(16, 24).to(torch.float16), r=8)):
        assert mod._use_hip(FakeCuda()) is False
        mod.hip = True
        with pytest.raises(_lib.MraError):
            mod._use_hip(FakeCuda())
        mod.hip = False
        assert mod._use_hip(FakeCuda()) is False


# ---- the trainer on a CPU model with a stub LM -----------------------------------------------------------------------------------------------
def test_trainer_saves_and_restores_the_adapters(tmp_path):
    from test_trainer_cpu import Narrow, TinyScorer
    from mraudio_amd.models.xinstructblip import XInstructBLIP
    from mraudio_amd.utils.trainer import Trainer, default_args

    class StubLM(nn.Module):
        def __init__(self):
            super().__init__()
            torch.manual_seed(1)
            self.proj, self.lm_head = nn.Linear(16, 16), nn.Linear(16, 4)

        def forward(self, x):
            return self.lm_head(torch.tanh(self.proj(x)))

    class WithLM(TinyScorer):
        lora = False
        enable_lora, lora_parameters, load_state_dict, train = (XInstructBLIP.enable_lora, XInstructBLIP.lora_parameters,
                                                                XInstructBLIP.load_state_dict, XInstructBLIP.train)
        modalities = []

        def __init__(self):
            super().__init__()
            object.__setattr__(self, "llm_model", StubLM())

        def forward(self, samples):
            out = super().forward(samples)
            lm = self.llm_model(samples["video_embeds"].mean(2)).pow(2).mean()
            return {"loss": out["loss"] + lm}

    data = dict(train_dataset=Narrow(4, T=20, seed=0, kv_video=2, modalities=("video",), signal=2.0),
                val_dataset=Narrow(2, T=20, seed=1, kv_video=2, modalities=("video",), signal=2.0))
    kw = dict(output_dir=str(tmp_path), gpu="cpu", lr=1e-2, warmup_steps=1, objective="both", lora=True, lora_r=4, lora_alpha=8, lora_dropout=0.0)
    with pytest.raises(ValueError, match="objective"):
        Trainer(default_args(max_epoch=1, **{**kw, "objective": "score"}), model=WithLM(), **data)
    model = WithLM()
    tr = Trainer(default_args(max_epoch=2, **kw), model=model, **data)
    assert model.lora and isinstance(model.llm_model.proj, L.LoraLinear) and isinstance(model.llm_model.lm_head, nn.Linear)
    opt_params = {id(p) for g in tr.optimizer.param_groups for p in g["params"]}
    assert {id(p) for p in model.lora_parameters()} <= opt_params
    tr.train()
    path = os.path.join(tmp_path, "checkpoint_1.pth")
    ck = torch.load(path, weights_only=True)["model"]
    kA, kB = ("llm_model.base_model.model.proj.lora_A.default.weight", "llm_model.base_model.model.proj.lora_B.default.weight")
    assert kA in ck and kB in ck and ck[kB].abs().sum() > 0 and "w.weight" in ck
    assert sorted(k for k in ck if k.startswith("llm_model")) == [kA, kB]
    saved = ck[kB].clone()
    with torch.no_grad():
        model.llm_model.proj.lora_B["default"].weight.zero_()
    tr2 = Trainer(default_args(max_epoch=3, resume_ckpt_path=path, **kw), model=model, **data)
    tr2._load_checkpoint(path)
    assert tr2.start_epoch == 2 and torch.equal(model.llm_model.proj.lora_B["default"].weight.detach(), saved)
    # without the switch the checkpoint is what it was: no llm_model.* key
    plain = Trainer(default_args(max_epoch=1, output_dir=str(tmp_path / "plain"), gpu="cpu"), model=TinyScorer(), **data)
    assert not plain.lora
    plain.train()
    assert not any(k.startswith("llm_model") for k in torch.load(os.path.join(tmp_path, "plain", "checkpoint_0.pth"), weights_only=True)["model"])


# ---- the CLI -----------------------------------------------------------------------------------------------------------------------------------
def test_cli_flags_parse_and_default_to_off(capsys):
    from mraudio_amd import evaluate, finetune

    base = ["--output-dir", "out", "--dataset", "QVH"]
    a = finetune.build_parser().parse_args(base)
    assert (a.lora, a.lora_r, a.lora_alpha, a.lora_dropout, a.train_qformers) == (False, 8, 8.0, 0.05, True)
    a = finetune.build_parser().parse_args(base + ["--lora", "--lora-r", "4", "--lora-alpha", "16", "--lora-dropout", "0.1", "--freeze-qformers",
                                                   "--objective", "llm", "--llm-path", "some/dir"])
    assert (a.lora, a.lora_r, a.lora_alpha, a.lora_dropout, a.train_qformers) == (True, 4, 16.0, 0.1, False)
    for extra in (["--lora"], ["--lora", "--llm-path", "some/dir"]):          # no LM, or the scorer objective
        with pytest.raises(SystemExit) as e:
            finetune.main(base + extra)
        assert e.value.code == 2 and "--lora needs" in capsys.readouterr().err
    e_ = evaluate.build_parser().parse_args(["--output-file", "o"])
    assert (e_.lora, e_.llm_path) == (False, None)
    e_ = evaluate.build_parser().parse_args(["--output-file", "o", "--lora", "--llm-path", "d", "--checkpoint", "f.pth"])
    assert e_.lora and e_.llm_path == "d"
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--output-file", "o", "--lora"])
    assert e.value.code == 2
