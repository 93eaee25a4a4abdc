"""Shared inputs of the prompt-plan tests (``test_prompt_plan_cpu.py``, ``test_gpu_prompt_rows.py``): a seeded embedding table behind
``SimpleLlmTokenizer``, batches whose tokenisation pads INSIDE the prefix (timestamps of one and three digits, durations of two and three),
ragged prompts and answers, a prompt cut from the left at ``max_txt_len`` and an answer cut at ``max_output_txt_len``, and the grouped
layout of ``forward_multi_train`` (chain row ``(k * T + pos) * P + p``)."""
import itertools

import torch

Q = 32
STAMPS = [3, 120, 7, 250, 9]                     # one and three digits in one row
PROMPTS = ["Query: a dog.\nWindows: ", "Query: a person opens the door and leaves.\nRelevant windows: ", "Q: x\nA: "]
ANSWERS = ["[[1, 2]]", "[[0, 3], [10, 12.5], [20, 31]]", "[[7, 9]]"]        # the second is cut at max_output_txt_len = 16
DURATIONS = [10, 100, 7]

MATRIX = list(itertools.product(("video", "audio", "both"), (False, True), (False, True), (1, 2, 3), (1, 2, 5),
                                (torch.bfloat16, torch.float16)))


def matrix_id(case):
    mods, enum, secs, B, T, dt = case
    return f"{mods}-enum{int(enum)}-secs{int(secs)}-B{B}-T{T}-{'bf16' if dt == torch.bfloat16 else 'f16'}"


def make_assembler(mods, enumerate_inputs, interleave_seconds, dtype, D=16, device="cpu", seed=0):
    from mraudio_amd.models.llm_prompt import PromptAssembler, SimpleLlmTokenizer

    tok = SimpleLlmTokenizer()
    torch.manual_seed(seed)
    emb = torch.nn.Embedding(len(tok), D).to(dtype).to(device).requires_grad_(False)
    names = ("video", "audio") if mods == "both" else (mods,)
    asm = PromptAssembler(tok, emb, modalities=names, num_query_token=Q, enumerate_inputs=enumerate_inputs,
                          interleave_seconds=interleave_seconds, max_txt_len=40, max_output_txt_len=16, device=device)
    return asm, emb


def make_samples(B, T, shift=0):
    return {"text_input": [PROMPTS[(b + shift) % 3] for b in range(B)], "text_output": [ANSWERS[(b + shift) % 3] for b in range(B)],
            "timestamps": [[STAMPS[(b + t) % 5] for t in range(T)] for b in range(B)], "duration": [DURATIONS[(b + shift) % 3] for b in range(B)]}


def make_media(names, rows, D, seed=1, device="cpu"):
    """fp32 projections whose values are spread over the 16-bit types' rounding (not representable in either)."""
    g = torch.Generator().manual_seed(seed)
    return {m: (torch.randn(rows, D, generator=g) * 3.0).to(device) for m in names}


def cat_forward(asm, samples, media, B, T, generate=False):
    """The cat route over fp32 projections that require a gradient: ``(embeds, mask, targets, leaves)``."""
    leaves = {m: v.detach().clone().view(B, T * Q, -1).requires_grad_(True) for m, v in media.items()}
    atts = {m: torch.ones(B, T * Q, dtype=torch.long, device=v.device) for m, v in leaves.items()}
    if generate:
        embeds, mask = asm.assemble_generate(samples, leaves, atts)
        return embeds, mask, None, leaves
    embeds, mask, targets = asm.assemble_forward(samples, leaves, atts)
    return embeds, mask, targets, leaves


# ---- the grouped layout: counts (3, 1, 2) padded to P = 3, T = 2 --------------------------------------------------------------------------
G_COUNTS, G_P, G_T = (3, 1, 2), 3, 2


def grouped_case():
    """``(flat_samples, pairs, media_rows, rows)``: one flattened sample per real (video, query) pair, in (video, query) order."""
    pairs = [(k, p) for k, c in enumerate(G_COUNTS) for p in range(c)]
    flat = {"text_input": [PROMPTS[(k + p) % 3] for k, p in pairs], "text_output": [ANSWERS[(k + 2 * p) % 3] for k, p in pairs],
            "timestamps": [[STAMPS[(k + t) % 5] for t in range(G_T)] for k, _ in pairs], "duration": [DURATIONS[k % 3] for k, _ in pairs]}

    def media_rows(seq, pos):
        k, p = pairs[seq]
        return ((k * G_T + pos) * G_P + p) * Q

    return flat, pairs, media_rows, len(G_COUNTS) * G_T * G_P * Q


def grouped_pick(x, pairs):
    """The rows of the real pairs out of a grouped projection ``[nb * T * P * Q, D]``, in the flattened batch's ordinary layout."""
    v = x.view(len(G_COUNTS), G_T, G_P, Q, -1)
    return torch.stack([v[k, :, p] for k, p in pairs]).reshape(len(pairs) * G_T * Q, -1)
