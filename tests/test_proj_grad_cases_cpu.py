"""CPU side of tests/proj_grad_cases.py: every faithful fp32 emulation of ``mra_llm_proj_backward`` sits inside its derived bound at every
shape the GPU test runs, every named mutant sits outside on at least one case of the table (the ratios are printed), the table covers what
it claims, the two new ABI entries are exported and refuse a NULL handle, and the host wiring of the LM objective (``finetune`` options,
``Trainer``, the differentiability of ``PromptAssembler.assemble_forward``) holds without a device."""
import ctypes as C

import pytest
import torch

import proj_grad_cases as PG
from mraudio_amd import _lib


def _id(dtype):
    return str(dtype).split(".")[-1]


def test_table_covers_row_residues_and_k_step_counts():
    seen = {(r % 128, lh // 64) for r, lh, _ in PG.cases()}
    for residue in (0, 1, 127):
        steps = {s for (res, s) in seen if res == residue}
        assert 1 in steps and 2 in steps, (residue, steps)                       # one and two K steps
        assert any(s % 2 == 1 and s > 1 for s in steps), (residue, steps)      # an odd number of them
        assert any(s >= 4 for s in steps), (residue, steps)                    # many
    assert PG.BIG in PG.cases() and sum(1 for _, lh, _ in PG.cases() if lh == 4096) == 1
    assert all(lh % 64 == 0 and h % 128 == 0 for _, lh, h in PG.cases())


@pytest.mark.parametrize("dout_f32", (True, False), ids=("dout_f32", "dout_op"))
@pytest.mark.parametrize("dtype", PG.DTYPES, ids=_id)
def test_emulations_sit_inside_their_bounds(dtype, dout_f32):
    worst = 0.0
    for rows, Lh, H in PG.cases():
        c = PG.make_proj(rows, Lh, H, dtype, dout_f32)
        ref, bound = PG.dz_ref(c["d_out"], c["W"])
        rz = PG.ratio(PG.dz_emulate(c["d_out"], c["W"]), ref, bound)
        splits = PG.tn_splits(rows, Lh, H)
        w_ref, w_b, b_ref, b_b = PG.dw_ref(c["d_out"], c["z"], dtype, c["dW0"], c["db0"], splits)
        dW, db = PG.dw_emulate(c["d_out"], c["z"], dtype, c["dW0"], c["db0"], splits)
        rw, rb = PG.ratio(dW, w_ref, w_b), PG.ratio(db, b_ref, b_b)
        print(f"proj bwd rows {rows} Lh {Lh} H {H} {_id(dtype)} f32 d_out {dout_f32}: d_z {rz:.3g} d_W {rw:.3g} d_b {rb:.3g}")
        assert max(rz, rw, rb) <= 1.0, (rows, Lh, H, rz, rw, rb)
        worst = max(worst, rz)
    assert worst > 0.0          # the emulation is fp32: it does not reproduce float64


def test_dz_walk_is_the_plain_product():
    """With values that are exact in fp32 sums (small integers) the tile walk of the emulation equals dY W bit for bit, and the reference
    is autograd of the float64 linear layer."""
    dy = torch.randint(-3, 4, (257, 320)).to(torch.float16)
    W = torch.randint(-2, 3, (320, 256)).to(torch.float16)
    assert torch.equal(PG.dz_emulate(dy, W), dy.float() @ W.float())
    c = PG.make_proj(5, 128, 256, torch.bfloat16, True)
    z, Wd = c["z"].to(torch.bfloat16).double().requires_grad_(True), c["W"].double().requires_grad_(True)
    b = torch.zeros(128, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.linear(z, Wd, b).backward(c["d_out"].to(torch.bfloat16).double())
    w_ref, _, b_ref, _ = PG.dw_ref(c["d_out"], c["z"], torch.bfloat16, None, None, 1)
    for got, ref in ((z.grad, PG.dz_ref(c["d_out"], c["W"])[0]), (Wd.grad, w_ref), (b.grad, b_ref)):
        assert (got - ref).abs().max() <= 1e-12 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("dtype", PG.DTYPES, ids=_id)
@pytest.mark.parametrize("mutant", PG.DZ_MUTANTS)
def test_dz_mutants_land_outside_somewhere(mutant, dtype):
    outside = []
    for rows, Lh, H in PG.cases():
        c = PG.make_proj(rows, Lh, H, dtype, True)
        ref, bound = PG.dz_ref(c["d_out"], c["W"])
        r = PG.ratio(PG.dz_emulate(c["d_out"], c["W"], mutant), ref, bound)
        print(f"d_z mutant {mutant} rows {rows} Lh {Lh} H {H} {_id(dtype)}: ratio {r:.3g}")
        if r > 1.0:
            outside.append((rows, Lh))
    assert outside, mutant
    if mutant == "tail_rows":          # exactly the cases with a short last tile
        assert set(outside) == {(r, lh) for r, lh, _ in PG.cases() if r % 128}
    if mutant in ("last_k_step_dropped", "w_not_transposed"):
        assert len(outside) == len(PG.cases())


@pytest.mark.parametrize("dtype", PG.DTYPES, ids=_id)
def test_dw_mutant_lands_outside(dtype):
    for rows, Lh, H in PG.cases()[:8]:
        c = PG.make_proj(rows, Lh, H, dtype, True)
        splits = PG.tn_splits(rows, Lh, H)
        w_ref, w_b, _, _ = PG.dw_ref(c["d_out"], c["z"], dtype, c["dW0"], c["db0"], splits)
        dW, _ = PG.dw_emulate(c["d_out"], c["z"], dtype, c["dW0"], c["db0"], splits, "prefill_overwritten")
        assert PG.ratio(dW, w_ref, w_b) > 1.0, (rows, Lh)


# ---- the ABI entries without a device ---------------------------------------------------------------------------------------------------
def test_new_entries_are_exported_and_refuse_a_null_handle():
    L = _lib.lib()
    handle = C.CDLL(_lib.LIB_PATH)
    for n in ("mra_llm_proj_backward", "mra_llm_proj_backward_workspace_bytes"):
        assert hasattr(handle, n) and n in _lib.PROTOTYPES
    f = C.create_string_buffer(1 << 12)
    p = C.addressof(f)
    # mra_llm_proj_backward(h, z, rows, d_out, d_out_dtype, d_z, d_weight, d_bias, workspace, workspace_bytes, stream)
    assert L.mra_llm_proj_backward(None, p, 4, p, _lib.MRA_F32, p, p, p, p, 1 << 12, None) == -1 and b"null" in L.mra_last_error()
    assert L.mra_llm_proj_backward_workspace_bytes(None, 4, _lib.MRA_F32) == 0


# ---- host wiring of the LM objective ----------------------------------------------------------------------------------------------------
def test_finetune_takes_the_objective_options_and_wants_an_llm_path(capsys):
    from mraudio_amd import finetune

    base = ["--output-dir", "out", "--dataset", "QVH"]
    a = finetune.build_parser().parse_args(base)
    assert (a.objective, a.lm_weight, a.train_proj, a.llm_path) == ("score", 1.0, False, None)
    a = finetune.build_parser().parse_args(base + ["--objective", "both", "--lm-weight", "0.5", "--train-proj", "--llm-path", "some/dir"])
    assert (a.objective, a.lm_weight, a.train_proj, a.llm_path) == ("both", 0.5, True, "some/dir")
    for obj in ("llm", "both"):
        with pytest.raises(SystemExit) as e:          # an argparse error, before anything touches a device
            finetune.main(base + ["--objective", obj])
        assert e.value.code == 2 and "--llm-path" in capsys.readouterr().err


def test_trainer_refuses_the_lm_objective_without_an_lm(tmp_path):
    from test_trainer_cpu import Narrow, TinyScorer
    from mraudio_amd.utils.trainer import Trainer, default_args

    data = dict(train_dataset=Narrow(4, T=20, seed=0, kv_video=2, modalities=("video",), signal=2.0),
                val_dataset=Narrow(2, T=20, seed=1, kv_video=2, modalities=("video",), signal=2.0))
    for obj in ("llm", "both"):
        with pytest.raises(RuntimeError, match="LM attached"):
            Trainer(default_args(output_dir=str(tmp_path), gpu="cpu", max_epoch=1, objective=obj), model=TinyScorer(), **data)
    with pytest.raises(ValueError, match="objective"):
        Trainer(default_args(output_dir=str(tmp_path), gpu="cpu", max_epoch=1, objective="lm"), model=TinyScorer(), **data)
    tr = Trainer(default_args(output_dir=str(tmp_path), gpu="cpu", max_epoch=1), model=TinyScorer(), **data)     # the default is the scorer loss
    assert tr.objective == "score" and tr.train_proj is False


def test_lm_loss_is_differentiable_in_inputs_llm():
    """What the LM objective relies on: the loss of ``assemble_forward`` + a stock Llama has a finite, non-zero gradient with respect to
    the projections handed to it."""
    tf = pytest.importorskip("transformers")
    from mraudio_amd.models.llm_prompt import PromptAssembler, SimpleLlmTokenizer

    torch.manual_seed(0)
    tok = SimpleLlmTokenizer()
    cfg = tf.LlamaConfig(vocab_size=len(tok), hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                         num_key_value_heads=4, max_position_embeddings=2048, pad_token_id=tok.pad_token_id, bos_token_id=2, eos_token_id=2)
    llm = tf.LlamaForCausalLM(cfg).eval().requires_grad_(False)
    asm = PromptAssembler(tok, llm.get_input_embeddings(), num_query_token=32)
    inputs = {m: torch.randn(2, 3 * 32, 64, requires_grad=True) for m in ("video", "audio")}
    atts = {m: torch.ones(2, 3 * 32, dtype=torch.long) for m in ("video", "audio")}
    samples = {"text_input": ["Query: a dog.\nRelevant windows: ", "Query: b\n"], "text_output": ["[[1, 2]]", "[[3, 4]]"],
               "timestamps": [[0, 1, 2], [3, 4, 5]], "duration": [10, 20]}
    e, m, t = asm.assemble_forward(samples, inputs, atts)
    loss = llm(inputs_embeds=e, attention_mask=m, labels=t, return_dict=True).loss
    loss.backward()
    assert torch.isfinite(loss)
    for m_, v in inputs.items():
        assert v.grad is not None and torch.isfinite(v.grad).all() and v.grad.abs().sum() > 0, m_
    assert all(p.grad is None for p in llm.parameters())
