"""Entry point with the reference's ``finetune.py`` flags (``:9-62``): one process per GPU under
``python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 -m mraudio_amd.finetune ...``
(RCCL through backend "nccl"); a single process when RANK / WORLD_SIZE are not set.

    python -m mraudio_amd.finetune --dataset Charades_STA --synthetic 16 --max-epoch 2 --output-dir out/ft
"""
from __future__ import annotations

import argparse
import datetime
import logging
import os

import torch
import torch.distributed as dist

from .utils.trainer import Trainer


def init_distributed_mode(args) -> None:
    """Reference ``finetune.py:9-31`` (SLURM branch dropped: one node, torchrun-style env only)."""
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ:
        args.rank, args.world_size, args.gpu = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ["LOCAL_RANK"])
    else:
        args.rank, args.world_size, args.gpu = 0, 1, 0
    torch.cuda.set_device(args.gpu)
    if args.world_size > 1:
        dist.init_process_group(backend="nccl", init_method="env://", world_size=args.world_size, rank=args.rank,
                                timeout=datetime.timedelta(minutes=30), device_id=torch.device("cuda", args.gpu))
        dist.barrier()


def run_train(args):
    init_distributed_mode(args)
    trainer = Trainer(args, model=build_llm_model(args) if args.llm_path else None)
    out = trainer.train()
    if args.rank == 0:
        print({"history": trainer.history, **out})
    if dist.is_initialized():
        dist.destroy_process_group()
    return out


def build_llm_model(args):
    """The model as ``Trainer`` would build it, with the causal LM of ``--llm-path`` attached: a LOCAL directory (``local_files_only``,
    never a hub name), loaded in the trainer's operand dtype (bf16), every LM parameter frozen."""
    from transformers import AutoModelForCausalLM, AutoTokenizer

    from .models.xinstructblip import XInstructBLIP
    if not os.path.isdir(args.llm_path):
        raise SystemExit(f"--llm-path {args.llm_path!r} is not a local directory (hub names are not fetched)")
    dev = torch.device("cuda", args.gpu)
    llm = AutoModelForCausalLM.from_pretrained(args.llm_path, local_files_only=True, torch_dtype=torch.bfloat16).to(dev)
    tok = AutoTokenizer.from_pretrained(args.llm_path, local_files_only=True, use_fast=False)
    llm.requires_grad_(False)
    model = XInstructBLIP(args.model_path, args.audio_encoder, device=dev, op_dtype=torch.bfloat16, checkpoint=args.checkpoint,
                          checkpoint_strict=not args.partial_checkpoint, cross_precision=args.cross_precision,
                          llm_hidden_size=llm.get_input_embeddings().weight.shape[1])
    model.attach_llm(llm, tok)
    return model       # --lora: Trainer calls model.enable_lora (after the bf16 cast above, so the adapters stay fp32 masters)


def build_parser() -> argparse.ArgumentParser:
    from .models.xinstructblip import LM_DECODES, LM_PREFILLS

    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="X-InstructBLIP")
    ap.add_argument("--model-path", default=None)
    ap.add_argument("--audio-encoder", default=None)
    ap.add_argument("--checkpoint", default=None, help="initial weights: state dict (.pth, reference key names)")
    ap.add_argument("--partial-checkpoint", action="store_true", help="accept a checkpoint that holds only part of the parameters (e.g. the trainer's trainable-only files); what it lacks keeps the seeded init and is reported")
    ap.add_argument("--video-folder", default=None)
    ap.add_argument("--train-annotation-file", default=None)
    ap.add_argument("--val-annotation-file", default=None)
    ap.add_argument("--embeds-folder", default=None)
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--val-freq", type=int, default=1)
    ap.add_argument("--save-freq", type=int, default=1)
    ap.add_argument("--max-epoch", type=int, default=50)
    ap.add_argument("--batch-size", type=int, default=1)
    ap.add_argument("--num-workers", type=int, default=0)
    ap.add_argument("--dataset", required=True, choices=["QVH", "Charades_STA"])
    ap.add_argument("--synthetic", type=int, default=0)
    ap.add_argument("--synthetic-queries", type=int, default=1, help="with --synthetic: queries per synthetic video (several make --group-by-video groups)")
    ap.add_argument("--group-by-video", action="store_true",
                    help="train on one record per video with all its queries: the encoders, the modality LayerNorm and the K/V projection run once per "
                         "video, the Q-Former layer chain once per query (XInstructBLIP.forward_multi); validation is unchanged")
    ap.add_argument("--max-queries-per-call", type=int, default=8, help="with --group-by-video: most queries of one video in one Q-Former call (at most 14)")
    ap.add_argument("--train-ln", action="store_true",
                    help="train the modality LayerNorms ({m}_ln) in front of the Q-Formers too (XInstructBLIP.enable_qformer_training(train_ln=True)); "
                         "the checkpoints then carry {m}_ln.*")
    ap.add_argument("--objective", default="score", choices=["score", "llm", "both"],
                    help="training loss: score (the build-defined scorer BCE), llm (the LM's cross-entropy on the answer tokens, the reference's "
                         "objective, through {m}_llm_proj into the Q-Formers) or both (bce + lm-weight * lm); validation stays on the scorer")
    ap.add_argument("--lm-weight", type=float, default=1.0, help="with --objective both: weight of the LM term")
    ap.add_argument("--train-proj", action="store_true",
                    help="train the projections into the LM ({m}_llm_proj) too (XInstructBLIP.enable_qformer_training(train_proj=True)); "
                         "the checkpoints then carry {m}_llm_proj.*")
    ap.add_argument("--llm-path", default=None, help="local directory of the causal LM (loaded with local_files_only, frozen, bf16); "
                                                     "required by --objective llm / both")
    ap.add_argument("--lora", action="store_true",
                    help="train LoRA adapters on every linear of the LM except lm_head (the reference's trainable set; HIP low-rank forward and "
                         "backward); needs --llm-path and --objective llm / both; the checkpoints then carry llm_model.*lora_{A,B}*")
    ap.add_argument("--lora-r", type=int, default=8, help="with --lora: the rank (at most 16)")
    ap.add_argument("--lora-alpha", type=float, default=8.0, help="with --lora: the scale is lora-alpha / lora-r")
    ap.add_argument("--lora-dropout", type=float, default=0.05, help="with --lora: dropout on the adapter branch's input, in [0, 1)")
    ap.add_argument("--freeze-qformers", dest="train_qformers", action="store_false",
                    help="keep the Q-Formers frozen (with --lora: the reference's step, only the adapters train)")
    ap.add_argument("--lm-loss", choices=("stock", "rows", "fused"), default="stock",
                    help="how the LM loss is computed: stock = the LM's own forward with labels (lm_head over every position); rows = the LM's "
                         "decoder, then lm_head + cross-entropy on the labelled rows only (torch ops); fused = the same on the HIP entries "
                         "mra_lm_head_ce_* (no [B, S, V] tensor in either direction); rows / fused need --objective llm or both")
    ap.add_argument("--prompt-assembly", choices=("cat", "plan"), default="cat",
                    help="how the prompt in front of the LM is put together: cat = torch.cat of its pieces; plan = a table of (source, row) "
                         "executed as one row gather forward and one per modality backward (mra_gather_rows); plan needs --objective llm or "
                         "both; --group-by-video with an LM objective always takes the plan")
    ap.add_argument("--val-decode", choices=("score", "llm"), default="score",
                    help="what validation scores: score = the scorer's span (as always); llm = the strings the attached LM decodes (generate_llm, "
                         "the reference's own validation); llm needs --llm-path")
    ap.add_argument("--lm-decode", choices=LM_DECODES, default="stock",
                    help="how the LM decodes: stock = llm_model.generate as it comes; hip = the same greedy decode over a static cache with the "
                         "one-token attention on mra_decode_attention; hip_step = the LM's own prefill, then one mra_lm_step per token")
    ap.add_argument("--lm-prefill", choices=LM_PREFILLS, default="stock",
                    help="the prefill in front of that decode: stock = the LM's forward as it is configured; hip = its attention on "
                         "mra_prefill_attention under the key mask alone (needs --lm-decode hip or hip_step)")
    ap.add_argument("--lm-attention", choices=("stock", "hip"), default="stock",
                    help="the LM's attention in the training pass: stock = the LM's forward as it is configured (SDPA under the [S, S] mask); hip = "
                         "one autograd node on mra_prefill_attention / mra_prefill_attention_backward under the key mask alone (needs "
                         "--objective llm or both)")
    ap.add_argument("--video-on-device", dest="video_device", action="store_true",
                    help="decoded video goes to the GPU as uint8 frames and is cropped, resized, flipped and normalised there "
                         "(mra_video_frames_forward) instead of as float32 pixels made on the host")
    ap.add_argument("--video-augment", action="store_true",
                    help="train on the reference's video augmentation: one random resized crop (bicubic, area share 0.9 .. 1.0) and one random "
                         "horizontal flip per clip, then the cast to uint8 (on the host, or on the GPU with --video-on-device)")
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--warmup-steps", type=int, default=1000)
    ap.add_argument("--cross-precision", default="op", choices=["op", "split", "auto"],
                    help="precision of the Q-Formers' cross-attention score chain in the validation forwards (training always runs op): "
                         "op, split or auto (measured on the first forward after every weight update)")
    return ap


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.objective != "score" and not args.llm_path:
        parser.error(f"--objective {args.objective} needs --llm-path DIR")
    if args.lora and (args.objective == "score" or not args.llm_path):
        parser.error("--lora needs --llm-path DIR and --objective llm or both")
    if args.lm_loss != "stock" and args.objective == "score":
        parser.error("--lm-loss rows / fused needs --objective llm or both")
    if args.lm_attention != "stock" and args.objective == "score":
        parser.error("--lm-attention hip needs --objective llm or both")
    if args.prompt_assembly != "cat" and args.objective == "score":
        parser.error("--prompt-assembly plan needs --objective llm or both")
    if args.val_decode == "llm" and not args.llm_path:
        parser.error("--val-decode llm needs --llm-path DIR")
    logging.basicConfig(level=logging.INFO)
    return run_train(args)


if __name__ == "__main__":
    main()
