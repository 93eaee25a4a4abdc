"""The prompt plan without a GPU: ``PromptAssembler.plan_forward`` / ``plan_generate`` + ``assemble_plan(hip=False)`` against the cat route
(``assemble_forward`` / ``assemble_generate``) bit for bit -- embeds, mask, targets and the gradient of a random cotangent to every
projection -- the grouped layout, ``PromptPlan.validate`` and the refusals of ``mra_gather_rows`` (host checks: nothing is launched).
A gather has no rounding of its own, so every comparison is exact."""
import ctypes as C

import pytest
import torch

import prompt_plan_cases as K
from mraudio_amd._lib import MRA_BF16, MRA_F16, MRA_F32, MraError, lib, mra_rows_src
from mraudio_amd.models.llm_prompt import PromptPlan, assemble_plan

D = 16


def _names(mods):
    return ("video", "audio") if mods == "both" else (mods,)


@pytest.mark.parametrize("case", K.MATRIX, ids=K.matrix_id)
def test_plan_equals_the_cat_route_forward_and_backward(case):
    mods, enum, secs, B, T, dt = case
    asm, emb = K.make_assembler(mods, enum, secs, dt, D)
    samples = K.make_samples(B, T)
    media = K.make_media(_names(mods), B * T * K.Q, D)
    embeds, mask, targets, leaves = K.cat_forward(asm, samples, media, B, T)
    plan = asm.plan_forward(samples, num=T)
    assert plan.plan.dtype == torch.int32 and tuple(plan.plan.shape) == (B, embeds.shape[1], 2)
    mine = {m: v.detach().clone().requires_grad_(True) for m, v in media.items()}
    e2, m2, t2 = assemble_plan(plan, emb.weight, mine, hip=False)
    assert e2.dtype == dt and torch.equal(e2.view(torch.int16), embeds.view(torch.int16))
    assert m2.dtype == mask.dtype and torch.equal(m2, mask) and t2.dtype == targets.dtype and torch.equal(t2, targets)
    if secs and T > 1:                 # padding inside the prefix (a one-digit stamp beside a three-digit one): the pad token's table row
        last_media = int(torch.nonzero(plan.plan[0, :, 0] > 0).max())
        inside = (plan.mask[:, :last_media] == 0) & (plan.plan[:, :last_media, 0] == 0)
        assert inside.any() and (plan.plan[:, :last_media, 1][inside] == asm.tok.pad_token_id).all()
    cot = torch.randn(embeds.shape, generator=torch.Generator().manual_seed(2)).to(dt)
    embeds.backward(cot)
    e2.backward(cot)
    for m in leaves:
        assert mine[m].grad.dtype == torch.float32 and torch.equal(mine[m].grad, leaves[m].grad.view(-1, D)), m
        assert (plan.inverse[m] >= 0).all() and mine[m].grad.abs().sum().item() > 0


@pytest.mark.parametrize("case", [c for c in K.MATRIX if c[5] == torch.bfloat16 and c[4] != 2], ids=K.matrix_id)
def test_plan_generate_equals_assemble_generate(case):
    mods, enum, secs, B, T, dt = case
    asm, emb = K.make_assembler(mods, enum, secs, dt, D)
    samples = K.make_samples(B, T)
    media = K.make_media(_names(mods), B * T * K.Q, D)
    with torch.no_grad():
        embeds, mask, _, _ = K.cat_forward(asm, samples, media, B, T, generate=True)
    plan = asm.plan_generate(samples, num=T)
    e2, m2, t2 = assemble_plan(plan, emb.weight, media, hip=False)
    assert t2 is None and plan.targets is None
    assert torch.equal(e2.view(torch.int16), embeds.view(torch.int16)) and torch.equal(m2, mask)
    if B > 1:
        assert (mask[:, -1] == 1).all() and (mask == 0).any()       # left padding of the prompt


def test_answer_and_prompt_are_cut_where_the_cat_route_cuts_them():
    asm, emb = K.make_assembler("both", False, True, torch.bfloat16, D)
    plan = asm.plan_forward(K.make_samples(3, 2), num=2)
    labelled = (plan.targets != -100).sum(1).tolist()
    assert labelled == [len(K.ANSWERS[0]) + 1, 15, len(K.ANSWERS[2]) + 1]      # answer + eos; 16 tokens with the bos, cut before the eos
    assert (plan.targets[1] == asm.tok.eos_token_id).sum().item() == 0 and (plan.targets[0] == asm.tok.eos_token_id).sum().item() == 1
    # the text piece is 40 + 15 wide: the 62-token prompt cut from the left at max_txt_len = 40 (its bos is gone), then the cut answer
    assert (plan.mask[1, -55:] == 1).all() and (plan.targets[:, :-55] == -100).all() and (plan.targets[1, -15:] != -100).all()
    assert plan.plan[1, -55, 1].item() != asm.tok.bos_token_id and plan.plan[0, -55, 1].item() == asm.tok.bos_token_id


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_grouped_layout_is_the_single_query_assembly_of_every_pair(dt):
    asm, emb = K.make_assembler("both", False, True, dt, D)
    flat, pairs, media_rows, rows = K.grouped_case()
    media = K.make_media(("video", "audio"), rows, D, seed=4)
    plan = asm.plan_forward(flat, media_rows, K.Q, num=K.G_T, rows=rows).validate(len(asm.tok))
    mine = {m: v.detach().clone().requires_grad_(True) for m, v in media.items()}
    e2, m2, t2 = assemble_plan(plan, emb.weight, mine, hip=False)
    # the flattened batch over the picked rows, through the cat route
    picked = {m: K.grouped_pick(v, pairs) for m, v in media.items()}
    embeds, mask, targets, leaves = K.cat_forward(asm, flat, picked, len(pairs), K.G_T)
    assert torch.equal(e2.view(torch.int16), embeds.view(torch.int16)) and torch.equal(m2, mask) and torch.equal(t2, targets)
    # every sequence alone: the single-query assembly of its pair, position for position where the mask is on
    for i, (k, p) in enumerate(pairs):
        one = {key: [val[i]] for key, val in flat.items()}
        rows_i = {m: v.view(len(pairs), K.G_T * K.Q, D)[i] for m, v in picked.items()}
        with torch.no_grad():
            e1, m1, t1, _ = K.cat_forward(asm, one, rows_i, 1, K.G_T)
        assert torch.equal(e2[i][m2[i] == 1].view(torch.int16), e1[0][m1[0] == 1].view(torch.int16)), (k, p)
        assert torch.equal(t2[i][m2[i] == 1], t1[0][m1[0] == 1])
    cot = torch.randn(embeds.shape, generator=torch.Generator().manual_seed(3)).to(dt)
    embeds.backward(cot)
    e2.backward(cot)
    real = torch.zeros(len(K.G_COUNTS), K.G_T, K.G_P, K.Q, dtype=torch.bool)
    for k, p in pairs:
        real[k, :, p] = True
    real = real.view(-1)
    for m in mine:
        assert torch.equal((plan.inverse[m] >= 0), real), m               # padded slots: -1 in the inverse plan ...
        assert mine[m].grad[~real].abs().max().item() == 0.0              # ... and a zero gradient
        assert torch.equal(K.grouped_pick(mine[m].grad, pairs), leaves[m].grad.view(-1, D))


def test_validate_refuses_a_row_out_of_range_and_a_row_used_twice():
    asm, emb = K.make_assembler("video", False, True, torch.bfloat16, D)
    samples = K.make_samples(2, 2)
    good = asm.plan_forward(samples, num=2)
    assert good.validate(len(asm.tok)) is good
    with pytest.raises(MraError, match="outside"):
        asm.plan_forward(samples, lambda b, pos: (b * 2 + pos) * K.Q + 1, num=2).validate()          # the last block runs one row past the end
    with pytest.raises(MraError, match="used twice"):
        asm.plan_forward(samples, lambda b, pos: pos * K.Q, num=2).validate()                         # both sequences read video 0
    with pytest.raises(MraError, match="token id"):
        good.validate(table_rows=100)
    bad = PromptPlan(good.plan.clone(), good.mask, good.targets, good.modalities, good.rows)
    bad.plan[0, 0, 0] = 7
    with pytest.raises(MraError, match="source"):
        bad.validate()
    with pytest.raises(MraError, match="used twice"):
        assemble_plan(asm.plan_forward(samples, lambda b, pos: pos * K.Q, num=2), emb.weight, K.make_media(("video",), 2 * 2 * K.Q, D), hip=False)


def test_hip_true_names_why_the_entry_does_not_apply():
    asm, emb = K.make_assembler("video", False, True, torch.bfloat16, D)
    plan = asm.plan_forward(K.make_samples(1, 1), num=1)
    with pytest.raises(MraError, match="CUDA"):
        assemble_plan(plan, emb.weight, K.make_media(("video",), K.Q, D), hip=True)


# ---- the entry's host checks: every refusal comes before any launch, so none of this touches a GPU ----------------------------------------
def _call(out=0x1000, ldo=64, out_dtype=MRA_BF16, n_rows=4, width=64, srcs=((0x2000, 64, 10, MRA_F32),), n_src=None, plan=0x3000, null_srcs=False):
    arr = (mra_rows_src * max(len(srcs), 1))(*[mra_rows_src(*s) for s in srcs])
    n = len(srcs) if n_src is None else n_src
    rc = lib().mra_gather_rows(C.c_void_p(out), ldo, out_dtype, n_rows, width, None if null_srcs else C.cast(arr, C.POINTER(mra_rows_src)), n,
                               C.c_void_p(plan), C.c_void_p(0))
    return rc, lib().mra_last_error().decode()


REFUSALS = {
    "null out": dict(out=0),
    "null srcs": dict(null_srcs=True),
    "null plan": dict(plan=0),
    "null source ptr": dict(srcs=((0, 64, 10, MRA_F32),)),
    "no source": dict(n_src=0),
    "five sources": dict(srcs=((0x2000, 64, 10, MRA_F32),) * 5),
    "width 12": dict(width=12, ldo=16, srcs=((0x2000, 16, 10, MRA_F32),)),
    "width 0": dict(width=0),
    "out misaligned": dict(out=0x1008),
    "source misaligned": dict(srcs=((0x2004, 64, 10, MRA_F32),)),
    "out pitch misaligned": dict(ldo=68),
    "source pitch misaligned": dict(srcs=((0x2000, 66, 10, MRA_F32),)),
    "ldo < width": dict(ldo=56),
    "ld < width": dict(srcs=((0x2000, 56, 10, MRA_F32),)),
    "unknown out dtype": dict(out_dtype=3),
    "unknown source dtype": dict(srcs=((0x2000, 64, 10, 9),)),
    "f16 to bf16": dict(srcs=((0x2000, 64, 10, MRA_F16),)),
    "bf16 to f16": dict(out_dtype=MRA_F16, srcs=((0x2000, 64, 10, MRA_F32), (0x4000, 64, 10, MRA_BF16))),
    "negative n_rows": dict(n_rows=-1),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_gather_rows_refuses_before_any_launch(name):
    rc, msg = _call(**REFUSALS[name])
    assert rc == -1 and msg.startswith("gather_rows") and len(msg) > len("gather_rows: "), (name, rc, msg)


def test_gather_rows_of_no_rows_is_a_no_op():
    assert _call(n_rows=0)[0] == 0
    assert _call(n_rows=0, out=0, plan=0, null_srcs=True, width=3)[0] == 0       # whatever else is passed
