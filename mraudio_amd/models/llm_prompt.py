"""LLM prompt assembly: what the reference does between the hot path's output
(``inputs_llm[m]`` = ``{m}_llm_proj(last_hidden_state[:, :32])``, ``[B, T*32, D]``) and the Llama call.

Layout of the embedded sequence, per sample (reference ``models/xinstructblip.py:341-381`` for ``generate``,
``:541-595`` for ``forward``), with T temporal positions and both modalities::

    for pos in 0..T-1:   [ "(a) " enumeration ]                       only if enumerate_inputs (default off, :70)
                         cue(" video: ")  video queries [pos]  (32)
                         cue(" audio: ")  audio queries [pos]  (32)
                         " {timestamp[pos]} "                          if interleave_seconds (default on, :73)
    "{duration} "
    prompt tokens                                                      generate: stripped text, no special tokens
                                                                       forward : input ++ output[1:] ++ input padding

``forward`` additionally builds the labels: -100 on everything before the prompt, on the instruction part and
on padding; the answer tokens (``text_output + eos``) carry the loss (``:502-516,584-595``).

The LLM itself is a stock module and stays out of this package: the assembler takes a tokenizer with the
HuggingFace call signature and an ``embed(ids) -> [.., D]`` callable (``llm_model.get_input_embeddings()``).
Neither Vicuna weights nor the Llama sentencepiece model exist offline, so ``SimpleLlmTokenizer`` is the
stand-in vocabulary for tests and smoke runs; with real checkpoints pass ``LlamaTokenizer`` instead.
Parity: the reference's class cannot be imported here (LAVIS / peft / Vicuna absent) and holds no fixtures for
this step -> **unpinned**; the tests re-derive the layout index by index from the lines cited above.

Every row of the embedded sequence is a row of the LM's embedding table or a row of a modality's projection, so the same two layouts
also exist as tables of integers: ``PromptAssembler.plan_forward`` / ``plan_generate`` make the same tokenizer calls in the same order and
return a ``PromptPlan`` (``plan [B, S, 2]`` = (source, row), ``mask``, ``targets``, one inverse plan per modality), and ``assemble_plan``
executes it as ONE autograd node: one ``mra_gather_rows`` launch forward and one per projection backward (``csrc/prompt.hip``), or
``index_select`` / ``index_copy_`` on the torch route, which is the oracle of the tests.  ``media_rows(seq, pos)`` names the first
projection row of a sequence at a position, so the ``(video, position, prompt)`` row order of ``forward_multi_train`` needs no permuted copy.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from .._lib import MraError, check, current_stream, lib, mra_dtype, mra_rows_src, ptr

MODALITY_TO_CUE = {"video": " video: ", "audio": " audio: "}       # reference :206-209


class _Enc:
    def __init__(self, input_ids: torch.Tensor, attention_mask: torch.Tensor):
        self.input_ids, self.attention_mask = input_ids, attention_mask

    def to(self, device):
        return _Enc(self.input_ids.to(device), self.attention_mask.to(device))


class SimpleLlmTokenizer:
    """Offline stand-in for ``LlamaTokenizer`` with the special tokens the reference installs (``:141-145``:
    pad ``[PAD]``, bos = eos = unk = ``</s>``).  Bytes map to ids 3..258; ``</s>`` = 2, ``[PAD]`` = 259.
    Implements what the assembler and ``generate`` use: the call (padding to the longest on ``padding_side``,
    truncation on ``truncation_side``, ``add_special_tokens`` = one leading bos), ``eos_token``,
    ``pad_token_id``, ``batch_decode``."""

    eos_token, eos_token_id, bos_token_id, pad_token_id = "</s>", 2, 2, 259

    def __init__(self, padding_side: str = "right", truncation_side: str = "left"):
        self.padding_side, self.truncation_side = padding_side, truncation_side

    def __len__(self) -> int:
        return 260

    def _ids(self, text: str, add_special_tokens: bool) -> List[int]:
        out: List[int] = [self.bos_token_id] if add_special_tokens else []
        while text:
            if text.startswith(self.eos_token):
                out.append(self.eos_token_id)
                text = text[len(self.eos_token):]
            else:
                out.extend(3 + b for b in text[0].encode("utf-8"))
                text = text[1:]
        return out

    def __call__(self, text, padding=False, truncation=False, max_length=None, return_tensors="pt", add_special_tokens=True, **unused):
        texts = [text] if isinstance(text, str) else list(text)
        rows = [self._ids(t, add_special_tokens) for t in texts]
        if truncation and max_length is not None:
            rows = [(r[-max_length:] if self.truncation_side == "left" else r[:max_length]) if len(r) > max_length else r for r in rows]
        width = max((len(r) for r in rows), default=0)
        ids = torch.full((len(rows), width), self.pad_token_id, dtype=torch.long)
        att = torch.zeros((len(rows), width), dtype=torch.long)
        for i, r in enumerate(rows):
            if not r:
                continue
            sl = slice(width - len(r), width) if self.padding_side == "left" else slice(0, len(r))
            ids[i, sl] = torch.tensor(r)
            att[i, sl] = 1
        return _Enc(ids, att)

    def batch_decode(self, ids, skip_special_tokens: bool = True) -> List[str]:
        out = []
        for row in torch.as_tensor(ids).tolist():
            text = b"".join(bytes([t - 3]) if 3 <= t <= 258 else (b"" if skip_special_tokens or t != self.eos_token_id else b"</s>")
                            for t in row)
            out.append(text.decode("utf-8", errors="ignore"))
        return out


def concat_text_input_output(input_ids, input_atts, output_ids, output_atts):
    """Per row: instruction tokens, then the answer without its leading bos, then the instruction's padding
    (reference ``:26-48``).  Returns the merged ``{"input_ids", "attention_mask"}`` and the instruction lengths."""
    lens, ids, atts = [], [], []
    for i in range(input_ids.size(0)):
        n = int(input_atts[i].sum())
        lens.append(n)
        ids.append(torch.cat([input_ids[i][:n], output_ids[i][1:], input_ids[i][n:]]))
        atts.append(torch.cat([input_atts[i][:n], output_atts[i][1:], input_atts[i][n:]]))
    return {"input_ids": torch.stack(ids), "attention_mask": torch.stack(atts)}, lens


class PromptAssembler:
    def __init__(self, llm_tokenizer, embed: Callable[[torch.Tensor], torch.Tensor], modalities: Sequence[str] = ("video", "audio"),
                 num_query_token: int = 32, enumerate_inputs: bool = False, interleave_seconds: bool = True, max_txt_len: int = 128,
                 max_output_txt_len: int = 64, device=None):
        self.tok, self.embed = llm_tokenizer, embed
        self.modalities = [m for m in ("video", "audio") if m in modalities]     # the reference interleaves in this order (:359)
        self.num_query_token = num_query_token
        self.enumerate_inputs, self.interleave_seconds = enumerate_inputs, interleave_seconds
        self.max_txt_len, self.max_output_txt_len = max_txt_len, max_output_txt_len
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        # cues are tokenised WITH special tokens (reference :215 uses the tokenizer's default), i.e. each carries a bos
        self.tokenized_cue: Dict[str, _Enc] = {}
        self.emb_cue: Dict[str, torch.Tensor] = {}
        for m in self.modalities:
            enc = self.tok(MODALITY_TO_CUE[m], return_tensors="pt")
            self.tokenized_cue[m] = enc
            with torch.no_grad():
                self.emb_cue[m] = self.embed(enc.input_ids.to(self.device))

    # ---- shared prefix: positions, duration ---------------------------------------------------------------
    def _prefix(self, samples, inputs_llm: Dict[str, torch.Tensor], atts_llm: Dict[str, torch.Tensor], n_prompts: int
                ) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
        dev, Q = self.device, self.num_query_token
        first = self.modalities[0]
        bs = inputs_llm[first].shape[0]
        num = {m: inputs_llm[m].shape[1] // Q for m in self.modalities}
        ts_emb = ts_att = None
        if self.interleave_seconds:
            flat = [f" {t} " for row in samples["timestamps"] for t in (row.tolist() if torch.is_tensor(row) else row)]
            tt = self.tok(flat, padding="longest", truncation=True, return_tensors="pt", add_special_tokens=False).to(dev)
            n_rows, per_row = len(samples["timestamps"]), len(samples["timestamps"][0])
            e = self.embed(tt.input_ids)
            ts_emb = e.view(n_rows, per_row, *e.shape[1:])
            ts_att = tt.attention_mask.view(n_rows, per_row, -1)
        inp: List[torch.Tensor] = []
        att: List[torch.Tensor] = []
        for pos in range(num[first]):
            if self.enumerate_inputs:
                en = self.tok([f"{'' if pos == 0 else ' '}({chr(97 + pos)}) " for _ in range(n_prompts)], return_tensors="pt",
                              add_special_tokens=pos == 0).to(dev)
                inp.append(self.embed(en.input_ids))
                att.append(en.attention_mask)
            for m in self.modalities:
                att.append(self.tokenized_cue[m].attention_mask.to(dev).repeat(bs, 1))
                att.append(atts_llm[m].view(bs, num[m], Q)[:, pos, :])
                inp.append(self.emb_cue[m].to(dev).repeat(bs, 1, 1))
                inp.append(inputs_llm[m].view(bs, num[m], Q, -1)[:, pos, :, :])
            if self.interleave_seconds:
                inp.append(ts_emb[:, pos, :, :])
                att.append(ts_att[:, pos, :])
        dur = self.tok([f"{d} " for d in samples["duration"]], padding="longest", truncation=True, return_tensors="pt",
                       add_special_tokens=False).to(dev)
        att.append(dur.attention_mask)
        inp.append(self.embed(dur.input_ids))
        return inp, att

    def _cat(self, inp: List[torch.Tensor], att: List[torch.Tensor]):
        dt = inp[-1].dtype
        return torch.cat([x.to(dt) for x in inp], dim=1), torch.cat(att, dim=1)

    # ---- generate (:309-381) --------------------------------------------------------------------------------
    def assemble_generate(self, samples, inputs_llm, atts_llm) -> Tuple[torch.Tensor, torch.Tensor]:
        self.tok.padding_side = "left"                               # :223
        prompt = [p.strip() for p in samples["text_input"]]          # :309
        llm = self.tok(prompt, padding="longest", return_tensors="pt", add_special_tokens=False).to(self.device)
        inp, att = self._prefix(samples, inputs_llm, atts_llm, len(prompt))
        att.append(llm.attention_mask)
        inp.append(self.embed(llm.input_ids))
        return self._cat(inp, att)

    # ---- forward (:481-595) -----------------------------------------------------------------------------------
    def assemble_forward(self, samples, inputs_llm, atts_llm) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        tok, dev = self.tok, self.device
        tok.padding_side, tok.truncation_side = "right", "left"
        tin = tok(samples["text_input"], return_tensors="pt", padding="longest", truncation=True, max_length=self.max_txt_len,
                  add_special_tokens=True).to(dev)
        tok.truncation_side = "right"
        tout = tok([t + tok.eos_token for t in samples["text_output"]], return_tensors="pt", padding="longest", truncation=True,
                   max_length=self.max_output_txt_len).to(dev)
        llm, in_len = concat_text_input_output(tin.input_ids, tin.attention_mask, tout.input_ids, tout.attention_mask)
        targets = llm["input_ids"].masked_fill(llm["input_ids"] == tok.pad_token_id, -100)
        for i, n in enumerate(in_len):
            targets[i][:n] = -100
        inp, att = self._prefix(samples, inputs_llm, atts_llm, len(samples["text_input"]))
        empty = torch.full(torch.cat(att, dim=1).size(), -100, dtype=torch.long, device=dev)
        att.append(llm["attention_mask"])
        inp.append(self.embed(llm["input_ids"]))
        embeds, mask = self._cat(inp, att)
        return embeds, mask, torch.cat([empty, targets], dim=1)

    # ---- the same two layouts as tables of integers (``PromptPlan``, ``assemble_plan``) ---------------------------------
    def _plan_prefix(self, samples, B: int, T: int, first_rows: torch.Tensor, Q: int, mods: Sequence[str]):
        """``_prefix`` on token ids: the same tokenizer calls in the same order, every piece a ``[B, L]`` triple (source, row, mask).
        Source 0 is the embedding table (row = token id, pad tokens included), source ``1 + i`` the projection of ``mods[i]``."""
        src: List[torch.Tensor] = []
        row: List[torch.Tensor] = []
        att: List[torch.Tensor] = []

        def tokens(ids, mask):
            src.append(torch.zeros_like(ids))
            row.append(ids)
            att.append(mask)

        ts_ids = ts_att = None
        if self.interleave_seconds:
            flat = [f" {t} " for r in samples["timestamps"] for t in (r.tolist() if torch.is_tensor(r) else r)]
            tt = self.tok(flat, padding="longest", truncation=True, return_tensors="pt", add_special_tokens=False)
            n_rows, per_row = len(samples["timestamps"]), len(samples["timestamps"][0])
            if n_rows != B or per_row < T:
                raise MraError(f"timestamps must hold one row of {T} stamps per sequence: got {n_rows} rows of {per_row} for {B} sequences")
            ts_ids = tt.input_ids.view(n_rows, per_row, -1)
            ts_att = tt.attention_mask.view(n_rows, per_row, -1)
        q = torch.arange(Q, dtype=torch.long)
        for pos in range(T):
            if self.enumerate_inputs:
                en = self.tok([f"{'' if pos == 0 else ' '}({chr(97 + pos)}) " for _ in range(B)], return_tensors="pt", add_special_tokens=pos == 0)
                tokens(en.input_ids, en.attention_mask)
            for i, m in enumerate(mods):
                cue = self.tokenized_cue[m]
                tokens(cue.input_ids.repeat(B, 1), cue.attention_mask.repeat(B, 1))
                src.append(torch.full((B, Q), 1 + i, dtype=torch.long))
                row.append(first_rows[:, pos, None] + q)
                att.append(torch.ones(B, Q, dtype=torch.long))
            if self.interleave_seconds:
                tokens(ts_ids[:, pos], ts_att[:, pos])
        dur = self.tok([f"{d} " for d in samples["duration"]], padding="longest", truncation=True, return_tensors="pt", add_special_tokens=False)
        tokens(dur.input_ids, dur.attention_mask)
        return src, row, att

    def _plan(self, samples, text_ids, text_att, targets, media_rows, n_query, num, rows, modalities) -> "PromptPlan":
        B = int(text_ids.shape[0])
        Q = int(n_query) if n_query is not None else self.num_query_token
        mods = [m for m in self.modalities if modalities is None or m in modalities]
        if not mods:
            raise MraError("a prompt plan needs at least one modality")
        T = int(num) if num is not None else len(samples["timestamps"][0])
        if media_rows is None:            # the ordinary layout: one contiguous [T * Q, D] block per sequence
            first = (torch.arange(B)[:, None] * T + torch.arange(T)[None, :]) * Q
        elif callable(media_rows):
            first = torch.tensor([[int(media_rows(b, pos)) for pos in range(T)] for b in range(B)], dtype=torch.long).view(B, T)
        else:
            first = torch.as_tensor(media_rows, dtype=torch.long).view(B, T)
        src, row, att = self._plan_prefix(samples, B, T, first, Q, mods)
        n_prefix = sum(int(a.shape[1]) for a in att)
        src.append(torch.zeros_like(text_ids))
        row.append(text_ids)
        att.append(text_att)
        src, row, mask = torch.cat(src, dim=1), torch.cat(row, dim=1), torch.cat(att, dim=1)
        if targets is not None:
            targets = torch.cat([torch.full((B, n_prefix), -100, dtype=torch.long), targets], dim=1)
        n_rows = {m: int(rows[m] if isinstance(rows, dict) else rows) if rows is not None else B * T * Q for m in mods}
        return PromptPlan(torch.stack([src, row], dim=2).to(torch.int32), mask, targets, mods, n_rows)

    def plan_generate(self, samples, media_rows=None, n_query: Optional[int] = None, *, num: Optional[int] = None, rows=None,
                      modalities: Optional[Sequence[str]] = None) -> "PromptPlan":
        """``assemble_generate`` as a ``PromptPlan``.  ``media_rows(seq, pos)`` (a callable or a ``[B, T]`` table; default the ordinary
        layout ``(seq * T + pos) * n_query``) is the first of the ``n_query`` projection rows of sequence ``seq`` at position ``pos``;
        ``num`` is T (default: the length of a ``timestamps`` row) and ``rows`` the row count of each projection (default ``B * T *
        n_query``; rows no sequence uses get -1 in the inverse plan)."""
        self.tok.padding_side = "left"
        prompt = [p.strip() for p in samples["text_input"]]
        llm = self.tok(prompt, padding="longest", return_tensors="pt", add_special_tokens=False)
        return self._plan(samples, llm.input_ids, llm.attention_mask, None, media_rows, n_query, num, rows, modalities)

    def plan_forward(self, samples, media_rows=None, n_query: Optional[int] = None, *, num: Optional[int] = None, rows=None,
                     modalities: Optional[Sequence[str]] = None) -> "PromptPlan":
        """``assemble_forward`` as a ``PromptPlan`` (arguments as ``plan_generate``); ``targets`` carries the labels."""
        tok = self.tok
        tok.padding_side, tok.truncation_side = "right", "left"
        tin = tok(samples["text_input"], return_tensors="pt", padding="longest", truncation=True, max_length=self.max_txt_len, add_special_tokens=True)
        tok.truncation_side = "right"
        tout = tok([t + tok.eos_token for t in samples["text_output"]], return_tensors="pt", padding="longest", truncation=True,
                   max_length=self.max_output_txt_len)
        llm, in_len = concat_text_input_output(tin.input_ids, tin.attention_mask, tout.input_ids, tout.attention_mask)
        targets = llm["input_ids"].masked_fill(llm["input_ids"] == tok.pad_token_id, -100)
        for i, n in enumerate(in_len):
            targets[i][:n] = -100
        return self._plan(samples, llm["input_ids"], llm["attention_mask"], targets, media_rows, n_query, num, rows, modalities)


class PromptPlan:
    """An assembled prompt as host integer tables: ``plan`` int32 [B, S, 2] = (source, row) per position (source 0 the LM's embedding table,
    ``1 + i`` the projection of ``modalities[i]``), ``mask`` [B, S], ``targets`` [B, S] (``plan_forward`` only) and per modality the inverse
    plan ``inverse[m]`` [rows_m]: the flat output row ``b * S + s`` that projection row lands on, or -1 for a row no sequence uses."""

    def __init__(self, plan: torch.Tensor, mask: torch.Tensor, targets: Optional[torch.Tensor], modalities: Sequence[str], rows: Dict[str, int]):
        self.plan, self.mask, self.targets = plan, mask, targets
        self.modalities, self.rows = list(modalities), dict(rows)
        flat = plan.view(-1, 2).to(torch.long)
        self.inverse: Dict[str, torch.Tensor] = {}
        self._used: Dict[str, torch.Tensor] = {}
        for i, m in enumerate(self.modalities):
            pos = torch.nonzero(flat[:, 0] == 1 + i).squeeze(1)
            self._used[m] = pos
            inv = torch.full((self.rows[m],), -1, dtype=torch.long)
            r = flat[pos, 1]
            ok = (r >= 0) & (r < self.rows[m])
            inv[r[ok]] = pos[ok]          # validate() refuses what this line cannot express: a row out of range or used twice
            self.inverse[m] = inv
        self._dev: Dict[torch.device, dict] = {}

    def validate(self, table_rows: Optional[int] = None) -> "PromptPlan":
        """Host check before upload: every source and row in range, every media row used at most once."""
        flat = self.plan.view(-1, 2).to(torch.long)
        s, r = flat[:, 0], flat[:, 1]
        if ((s < 0) | (s > len(self.modalities))).any():
            raise MraError(f"prompt plan: a source outside [0, {len(self.modalities)}]")
        tok = r[s == 0]
        if (tok < 0).any() or (table_rows is not None and (tok >= table_rows).any()):
            raise MraError(f"prompt plan: a token id outside the embedding table's {table_rows} rows")
        for i, m in enumerate(self.modalities):
            mr = r[s == 1 + i]
            if ((mr < 0) | (mr >= self.rows[m])).any():
                raise MraError(f"prompt plan: a {m} row outside [0, {self.rows[m]})")
            if torch.unique(mr).numel() != mr.numel():
                raise MraError(f"prompt plan: a {m} row is used twice (its gradient would need a sum)")
        if self.mask.shape != self.plan.shape[:2] or (self.targets is not None and self.targets.shape != self.mask.shape):
            raise MraError("prompt plan: plan, mask and targets disagree on [B, S]")
        return self

    def on(self, device) -> dict:
        """The device copies, uploaded once per device: ``plan`` int32 [B * S, 2], ``mask``, ``targets``, per modality ``inv`` int32
        [rows_m, 2] (the backward's plan over d_embeds; (-1, 0) = a zero row) and the index vectors of the torch route."""
        device = torch.device(device)
        d = self._dev.get(device)
        if d is None:
            flat = self.plan.view(-1, 2)
            is_tok = flat[:, 0] == 0
            d = {"plan": flat.contiguous().to(device), "mask": self.mask.to(device), "targets": None if self.targets is None else self.targets.to(device),
                 "tok_pos": torch.nonzero(is_tok).squeeze(1).to(device), "tok": flat[:, 1].to(torch.long).masked_fill(~is_tok, 0).to(device),
                 "inv": {}, "pos": {}, "row": {}}
            for m in self.modalities:
                inv = self.inverse[m]
                d["inv"][m] = torch.stack([torch.where(inv < 0, -1, 0), inv.clamp(min=0)], dim=1).to(torch.int32).contiguous().to(device)
                d["pos"][m] = self._used[m].to(device)
                d["row"][m] = flat[self._used[m], 1].to(torch.long).to(device)
            self._dev[device] = d
        return d


def gather_rows(srcs: Sequence[torch.Tensor], plan: torch.Tensor, out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None
                ) -> torch.Tensor:
    """``mra_gather_rows``: ``out[i] = cast(srcs[s][r])`` for ``plan[i] = (s, r)`` (int32 [n, 2] on the device); ``srcs`` are 2-D with unit
    column stride, pitched rows allowed.  ``out`` (pitched allowed) is allocated ``[n, width]`` of ``out_dtype`` when not given."""
    n, width = int(plan.shape[0]), int(srcs[0].shape[1])
    if out is None:
        out = torch.empty(n, width, dtype=out_dtype or srcs[0].dtype, device=plan.device)
    arr = (mra_rows_src * len(srcs))()
    for k, t in enumerate(srcs):
        if t.dim() != 2 or t.shape[1] != width or t.stride(1) != 1:
            raise MraError(f"gather_rows: source {k} must be [rows, {width}] with unit column stride, got {tuple(t.shape)} / {t.stride()}")
        arr[k] = mra_rows_src(t.data_ptr(), t.stride(0) if t.shape[0] > 1 else max(t.stride(0), width), t.shape[0], mra_dtype(t.dtype))
    if out.dim() != 2 or out.shape[0] != n or out.shape[1] != width or out.stride(1) != 1 or plan.dtype != torch.int32 or not plan.is_contiguous():
        raise MraError("gather_rows: out must be [n, width] with unit column stride and plan a contiguous int32 [n, 2]")
    check(lib().mra_gather_rows(ptr(out), out.stride(0) if n > 1 else max(out.stride(0), width), mra_dtype(out.dtype), n, width,
                                C.cast(arr, C.POINTER(mra_rows_src)), len(srcs), ptr(plan), current_stream()), "mra_gather_rows")
    return out


def _plan_hip_reason(table: torch.Tensor, media: Sequence[torch.Tensor]) -> Optional[str]:
    """None when ``mra_gather_rows`` applies, else why not."""
    if not table.is_cuda or not all(x.is_cuda for x in media):
        return "the table and the projections must be CUDA tensors"
    if table.requires_grad and torch.is_grad_enabled():
        return "the embedding table requires a gradient, which only the torch route computes"
    if table.shape[1] % 8:
        return f"width {table.shape[1]} is not a multiple of 8"
    if table.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        return f"unsupported table dtype {table.dtype}"
    for x in media:
        if x.dtype != torch.float32 and x.dtype != table.dtype:
            return f"a {x.dtype} projection into a {table.dtype} table (f32, or the table's own dtype)"
    per = 4 if table.dtype == torch.float32 else 8
    if table.stride(1) != 1 or table.stride(0) % per or table.stride(0) < table.shape[1] or table.data_ptr() % 16:
        return "the table is not laid out as the entry reads it (unit column stride, 16-byte aligned rows), and no copy of it is made"
    return None


class _AssemblePlan(torch.autograd.Function):
    """ONE node: the forward is one gather over (table, projections...), the backward one gather per projection that needs a gradient
    (``mra_gather_rows`` with d_embeds as the source and the inverse plan), or ``index_select`` / ``index_copy_`` on the torch route."""

    @staticmethod
    def forward(ctx, dev, mods, use_hip, table, *media):
        flat = [x.reshape(-1, x.shape[-1]) for x in media]
        if use_hip:
            flat = [x if x.stride(1) == 1 and x.stride(0) % (4 if x.dtype == torch.float32 else 8) == 0 and x.data_ptr() % 16 == 0 else x.contiguous()
                    for x in flat]
            out = gather_rows([table] + flat, dev["plan"], table.dtype)
        else:
            out = table.index_select(0, dev["tok"])
            for m, x in zip(mods, flat):
                out.index_copy_(0, dev["pos"][m], x.index_select(0, dev["row"][m]).to(table.dtype))
        ctx.dev, ctx.mods, ctx.use_hip = dev, mods, use_hip
        ctx.meta = (tuple(table.shape), table.dtype, [(tuple(x.shape), x.dtype) for x in media])
        return out

    @staticmethod
    def backward(ctx, g):
        dev, mods = ctx.dev, ctx.mods
        tshape, tdtype, minfo = ctx.meta
        g = g.reshape(-1, tshape[1])
        grads: List[Optional[torch.Tensor]] = []
        d_table = None
        if ctx.needs_input_grad[3]:
            d_table = torch.zeros(tshape, dtype=tdtype, device=g.device).index_add_(0, dev["tok"].index_select(0, dev["tok_pos"]),
                                                                                     g.index_select(0, dev["tok_pos"]))
        if ctx.use_hip and not (g.stride(1) == 1 and g.stride(0) % (4 if g.dtype == torch.float32 else 8) == 0 and g.data_ptr() % 16 == 0):
            g = g.contiguous()
        for k, (m, (shape, dtype)) in enumerate(zip(mods, minfo)):
            if not ctx.needs_input_grad[4 + k]:
                grads.append(None)
            elif ctx.use_hip:
                grads.append(gather_rows([g], dev["inv"][m], dtype).view(shape))
            else:
                d = torch.zeros(dev["inv"][m].shape[0], tshape[1], dtype=dtype, device=g.device)
                d.index_copy_(0, dev["row"][m], g.index_select(0, dev["pos"][m]).to(dtype))
                grads.append(d.view(shape))
        return (None, None, None, d_table, *grads)


def assemble_plan(plan: PromptPlan, table: torch.Tensor, media: Dict[str, torch.Tensor], hip: Optional[bool] = None):
    """Execute a plan: ``(embeds [B, S, D] in the table's dtype, mask, targets)`` on the table's device (``targets`` is None for a
    ``plan_generate`` plan).  ``table`` is the LM's embedding weight ``[V, D]``, ``media[m]`` the projection of modality ``m`` with
    ``plan.rows[m]`` rows of D in any leading shape, fp32 or the table's dtype; the cast to the table's dtype happens inside the gather.
    One autograd node; the gradient of a projection comes out in its own dtype.  ``hip=None`` takes ``mra_gather_rows`` when it applies
    (CUDA, D % 8 == 0, a table that needs no gradient) and the torch route (``index_select`` / ``index_copy_``) otherwise; ``hip=True``
    raises ``MraError`` naming the reason; ``hip=False`` is the torch route."""
    B, S = plan.mask.shape
    xs = []
    for m in plan.modalities:
        if m not in media:
            raise MraError(f"assemble_plan: the plan uses modality {m!r}, which media does not hold")
        x = media[m]
        if x.shape[-1] != table.shape[1] or x.numel() != plan.rows[m] * table.shape[1]:
            raise MraError(f"assemble_plan: {m} holds {tuple(x.shape)}, the plan expects {plan.rows[m]} rows of {table.shape[1]}")
        xs.append(x)
    plan.validate(int(table.shape[0]))
    use = False
    if hip is None or hip:
        why = _plan_hip_reason(table, xs)
        if why is not None and hip:
            raise MraError(f"assemble_plan(hip=True): {why}")
        use = why is None
    dev = plan.on(table.device)
    out = _AssemblePlan.apply(dev, tuple(plan.modalities), use, table, *xs)
    return out.view(B, S, table.shape[1]), dev["mask"], dev["targets"]
