"""Inference loop of the reference's ``evaluate.py:41-59``: batches -> ``model.generate`` -> span parsing ->
one JSON line per query, in the format ``eval/mr_eval.py`` (here ``mraudio_amd.eval.mr_eval``) scores.
On top of the reference's record this build also writes ``pred_saliency_scores`` -- the fused per-position
cosine logits the span was cut from -- so the highlight metrics can be computed as well.  With ``--top-k N`` (N > 1)
``pred_relevant_windows`` is the ranked list of up to N ``[start_s, end_s, score]`` proposals (``model.generate_windows``).

    python -m mraudio_amd.evaluate --synthetic 8 --output-file out/pred.jsonl      # smoke run on the GPU
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Iterable, List, Optional

import torch

from .utils.mr_dataset import prepare_sample
from .utils.spans import moment_str_to_list, post_process


@torch.no_grad()
def run_inference(model, dataloader: Iterable[dict], output_file: Optional[str] = None, with_saliency: bool = True,
                  device=None, top_k: int = 1, use_llm: bool = False) -> List[dict]:
    records: List[dict] = []
    fh = None
    if output_file:
        os.makedirs(os.path.dirname(os.path.abspath(output_file)), exist_ok=True)
        fh = open(output_file, "w")
    for samples in dataloader:
        samples = prepare_sample(samples, device)
        scores = windows = None
        if use_llm:     # the reference's own decode: the attached LM (with its LoRA adapters, in eval mode) writes the answer
            outputs = model.generate_llm(samples)
        elif top_k > 1:   # ranked proposals: [start_s, end_s, score] triples in rank order, raw_out the multi-window string
            outputs, windows, scores = model.generate_windows(samples)
            if not with_saliency:
                scores = None
        elif with_saliency and hasattr(model, "generate_with_scores"):
            outputs, scores = model.generate_with_scores(samples)
        else:
            outputs = model.generate(samples)
        for k, (qid, query, vid, raw) in enumerate(zip(samples["qid"], samples["query"], samples["vid"], outputs)):
            pred = windows[k] if windows is not None else moment_str_to_list(post_process(raw))
            rec = {"qid": qid, "query": query, "vid": vid, "pred_relevant_windows": pred, "raw_out": raw}
            if scores is not None:
                rec["pred_saliency_scores"] = [float(x) for x in scores[k]]
            records.append(rec)
            if fh:
                fh.write(json.dumps(rec) + "\n")
        if len(records) == len(outputs) and hasattr(model, "cross_precision_report"):   # once, after the first batch
            print(f"cross-attention precision: {format_cross_precision(model.cross_precision_report())}")
    if fh:
        fh.close()
    return records


@torch.no_grad()
def run_inference_grouped(model, dataloader: Iterable[dict], output_file: Optional[str] = None, with_saliency: bool = True,
                          device=None, top_k: int = 1) -> List[dict]:
    """``run_inference`` over ``VideoGroupedDataset`` batches: every video is encoded once and its queries are scored together
    (``model.generate_multi*``).  Same record per query, written in the annotation file's original order."""
    by_line = {}
    for samples in dataloader:
        samples = prepare_sample(samples, device)
        queries = samples["text_input"]
        scores = windows = None
        if top_k > 1:
            outputs, windows, scores = model.generate_multi_windows(samples, queries)
            if not with_saliency:
                scores = None
        elif with_saliency:
            outputs, scores = model.generate_multi_with_scores(samples, queries)
        else:
            outputs = model.generate_multi(samples, queries)
        first = not by_line
        for b, (lines, qids, qs, vid) in enumerate(zip(samples["index"], samples["qid"], samples["query"], samples["vid"])):
            for k, (line, qid, query) in enumerate(zip(lines, qids, qs)):
                raw = outputs[b][k]
                pred = windows[b][k] if windows is not None else moment_str_to_list(post_process(raw))
                rec = {"qid": qid, "query": query, "vid": vid, "pred_relevant_windows": pred, "raw_out": raw}
                if scores is not None:
                    rec["pred_saliency_scores"] = [float(x) for x in scores[b][k]]
                by_line[int(line)] = rec
        if first and hasattr(model, "cross_precision_report"):   # once, after the first batch
            print(f"cross-attention precision: {format_cross_precision(model.cross_precision_report())}")
    records = [by_line[i] for i in sorted(by_line)]
    if output_file:
        os.makedirs(os.path.dirname(os.path.abspath(output_file)), exist_ok=True)
        with open(output_file, "w") as fh:
            for rec in records:
                fh.write(json.dumps(rec) + "\n")
    return records


def format_cross_precision(report: dict) -> str:
    """One line per model: for each modality the mode set, the precision in force and the probe's per-cross-layer median p_max."""
    parts = []
    for m, r in report.items():
        med = ", ".join(f"{x:.3f}" for x in r["median_pmax"]) if r["probes"] else "-"
        parts.append(f"{m}: {r['mode']} -> {r['resolved'] or 'unresolved'} (median p_max per cross layer: {med})")
    return "; ".join(parts)


def build_parser() -> argparse.ArgumentParser:
    from .models.xinstructblip import LM_DECODES, LM_PREFILLS

    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="X-InstructBLIP")
    ap.add_argument("--model-path", default=None)
    ap.add_argument("--audio-encoder", default=None)
    ap.add_argument("--checkpoint", default=None, help="state dict (.pth, reference key names) with the Q-Former / LN / projection weights")
    ap.add_argument("--partial-checkpoint", action="store_true", help="accept a checkpoint that holds only part of the parameters (e.g. the trainer's trainable-only files); what it lacks keeps the seeded init and is reported")
    ap.add_argument("--video-folder", default=None)
    ap.add_argument("--annotation-file", default=None)
    ap.add_argument("--embeds-folder", default=None, help="pre-extracted encoder outputs, <vid>.pt")
    ap.add_argument("--output-file", required=True)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--batch-size", type=int, default=2)
    ap.add_argument("--num-workers", type=int, default=0)
    ap.add_argument("--dataset", default="Charades_STA", choices=["QVH", "Charades_STA"])
    ap.add_argument("--synthetic", type=int, default=0, help="evaluate N seeded synthetic videos instead of a corpus")
    ap.add_argument("--cross-precision", default="op", choices=["op", "split", "auto"],
                    help="precision of the Q-Formers' cross-attention score chain: op (f16 / bf16 operands), split (~22-bit hi + lo pairs, "
                         "+28 %% of the step) or auto (measured on the first batch after the weights are loaded: split for sharply attending weights)")
    ap.add_argument("--top-k", type=int, default=1, help="ranked proposals per query: N > 1 writes up to N [start_s, end_s, score] windows in rank order "
                                                         "(top windows by summed excess over the span threshold under temporal NMS); 1 = the single span")
    ap.add_argument("--nms-thd", type=float, default=0.25, help="temporal IoU above which a proposal is suppressed by a higher-ranked one, in [0, 1)")
    ap.add_argument("--max-window", type=int, default=0, help="longest proposal in clips (0 = no cap)")
    ap.add_argument("--group-by-video", action="store_true",
                    help="encode every video once and score its queries together over one shared K/V cache (same records, annotation order)")
    ap.add_argument("--max-queries-per-call", type=int, default=16, help="with --group-by-video: most queries of one video scored in one call")
    ap.add_argument("--llm-path", default=None, help="local directory of the causal LM (local_files_only, bf16): predictions then come from "
                                                     "generate_llm, the reference's decode")
    ap.add_argument("--lm-decode", choices=LM_DECODES[:2], default="stock",       # "hip_step" is --lm-step here
                    help="with --llm-path: how the LM decodes: stock = llm_model.generate as it comes; hip = the same greedy decode over a static "
                         "cache with the one-token attention on mra_decode_attention")
    ap.add_argument("--lm-step", action="store_true",
                    help="with --llm-path: decode as finetune's --lm-decode hip_step does: the LM's own prefill, then one mra_lm_step per token "
                         "(not together with --lm-decode hip)")
    ap.add_argument("--lm-prefill", choices=LM_PREFILLS, default="stock",
                    help="with --llm-path and --lm-decode hip or --lm-step: the prefill's attention on mra_prefill_attention under the key mask alone")
    ap.add_argument("--lora", action="store_true", help="with --llm-path: put LoRA adapters on the LM and load their weights (llm_model.* keys) from --checkpoint")
    ap.add_argument("--lora-r", type=int, default=8)
    ap.add_argument("--lora-alpha", type=float, default=8.0)
    ap.add_argument("--lora-dropout", type=float, default=0.05)
    ap.add_argument("--video-on-device", action="store_true",
                    help="decoded video goes to the GPU as uint8 frames and is normalised there (mra_video_frames_forward) instead of as float32 "
                         "pixels made on the host")
    return ap


def main(argv=None) -> None:
    from torch.utils.data import DataLoader

    from .models.xinstructblip import XInstructBLIP, check_lm_options
    from .utils.mr_dataset import MRDataset, SyntheticMRDataset, VideoGroupedDataset, collate_fn, collate_grouped

    parser = build_parser()
    args = parser.parse_args(argv)
    if args.lm_step and args.lm_decode != "stock":
        parser.error("--lm-step and --lm-decode hip name two different decodes: give one of them")
    if args.lm_prefill == "hip" and not (args.llm_path and (args.lm_step or args.lm_decode == "hip")):
        parser.error("--lm-prefill hip needs --llm-path DIR and a HIP decode (--lm-decode hip or --lm-step)")
    if args.lora and not args.llm_path:
        parser.error("--lora needs --llm-path DIR")
    if args.llm_path and (args.group_by_video or args.top_k > 1):
        parser.error("--llm-path decodes one answer per query: not with --group-by-video or --top-k")
    n_frms = 60 if args.dataset == "QVH" else 20
    vproc = None
    if args.video_on_device:
        from .processors.alpro_processors import AlproVideoEvalProcessor_Stamps
        vproc = AlproVideoEvalProcessor_Stamps(n_frms=n_frms, image_size=224, device=args.device)
    llm = tok = None
    if args.llm_path:
        from transformers import AutoModelForCausalLM, AutoTokenizer
        if not os.path.isdir(args.llm_path):
            raise SystemExit(f"--llm-path {args.llm_path!r} is not a local directory (hub names are not fetched)")
        llm = AutoModelForCausalLM.from_pretrained(args.llm_path, local_files_only=True, torch_dtype=torch.bfloat16).to(args.device).eval()
        tok = AutoTokenizer.from_pretrained(args.llm_path, local_files_only=True, use_fast=False)
        llm.requires_grad_(False)
    model = XInstructBLIP(args.model_path, args.audio_encoder, device=args.device, checkpoint=None if args.lora else args.checkpoint,
                          checkpoint_strict=not args.partial_checkpoint,
                          cross_precision=args.cross_precision, top_k=args.top_k, nms_thd=args.nms_thd, max_window=args.max_window,
                          **({} if vproc is None else {"video_processor": vproc}),
                          **({} if llm is None else {"op_dtype": torch.bfloat16, "llm_hidden_size": llm.get_input_embeddings().weight.shape[1]}))
    if llm is not None:
        model.attach_llm(llm, tok)
        lm_decode = "hip_step" if args.lm_step else args.lm_decode
        check_lm_options(lm_decode, args.lm_prefill)
        model.lm_decode, model.lm_prefill = lm_decode, args.lm_prefill
        if args.lora:       # the adapters must exist before the file's llm_model.* keys can be routed into them
            model.enable_lora(r=args.lora_r, alpha=args.lora_alpha, dropout=args.lora_dropout)
            if args.checkpoint:
                model.load_checkpoint(args.checkpoint, strict=not args.partial_checkpoint)
        model.eval()
    print(f"weights: {model.weights_source}")
    if args.synthetic:
        ds = SyntheticMRDataset(args.synthetic, T=n_frms)
    else:
        ds = MRDataset(args.video_folder, args.annotation_file, vproc, None, model=args.model, embeds_root=args.embeds_folder)
    if args.group_by_video:
        dl = DataLoader(VideoGroupedDataset(ds, args.max_queries_per_call), shuffle=False, batch_size=args.batch_size, num_workers=args.num_workers,
                        collate_fn=collate_grouped)
        recs = run_inference_grouped(model, dl, args.output_file, device=torch.device(args.device), top_k=args.top_k)
    else:
        dl = DataLoader(ds, shuffle=False, batch_size=args.batch_size, num_workers=args.num_workers, collate_fn=collate_fn)
        recs = run_inference(model, dl, args.output_file, device=torch.device(args.device), top_k=args.top_k, use_llm=llm is not None)
    print(f"wrote {len(recs)} predictions to {args.output_file}")


if __name__ == "__main__":
    main()
