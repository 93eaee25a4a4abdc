"""Moment-retrieval dataset with the reference's record layout (``utils/mr_dataset.py:7-119``).

A record is what ``XInstructBLIP.generate`` / ``forward`` read: ``text_input`` (the two-line prompt of
``:96-98``), ``text_output`` (``str(relevant_windows)``), ``video`` [C, T, H, W] (with a device video processor instead ``video_raw`` uint8 [T, H, W, 3], ``video_box`` int64 [4] and
``video_flip``: the decoded bytes and the clip's crop box and flip), ``audio`` [T, F, 128],
``timestamps`` (``round(index / fps)`` per sampled frame, ``:44``), ``duration``, ``qid``, ``query``, ``vid``.

Decoding is not part of the hot path and neither ffmpeg nor decord exists in this image, so the decoders
are the pluggable processors of ``mraudio_amd.processors``; clipping by ``start`` / ``end`` (the reference
shells out to ffmpeg, ``:25-35``) is handed to the processor as a keyword when it accepts one.  For a
corpus whose encoder outputs were extracted once, ``embeds_root`` replaces both processors: the record then
carries ``video_embeds`` [T, 257, 1408] / ``audio_embeds`` [T, Kv, 768] (what BASELINE configs 1-5 feed).
"""
from __future__ import annotations

import inspect
import json
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
from torch.utils.data import Dataset

QUERY_PREFIX = "Query: "
TASK_PROMPT = "Given the video and the query, find the relevant windows.\nRelevant windows: "


def build_prompt(query: str) -> str:
    """``utils/mr_dataset.py:96-98``."""
    return QUERY_PREFIX + query + "\n" + TASK_PROMPT


class MRDataset(Dataset):
    def __init__(self, vis_root: str, ann_path: str, video_processor: Optional[Callable], audio_processor: Optional[Callable],
                 model: str = "X-InstructBLIP", embeds_root: Optional[str] = None):
        self.vis_root, self.video_processor, self.audio_processor, self.model = vis_root, video_processor, audio_processor, model
        self.embeds_root = embeds_root
        with open(ann_path, "r") as f:
            self.annotation = [json.loads(line) for line in f if line.strip()]

    def __len__(self) -> int:
        return len(self.annotation)

    @staticmethod
    def _call(proc: Callable, path: str, ann: dict):
        if "start" in ann and "clip" in inspect.signature(proc.__call__ if not inspect.isfunction(proc) else proc).parameters:
            return proc(path, clip=(float(ann["start"]), float(ann["end"])))
        return proc(path)

    def __getitem__(self, index: int) -> Dict[str, object]:
        ann = self.annotation[index]
        rec: Dict[str, object] = {"text_input": build_prompt(ann["query"]), "text_output": str(ann["relevant_windows"]),
                                  "duration": ann["duration"], "qid": ann["qid"], "query": ann["query"], "vid": ann["vid"]}
        if self.embeds_root is not None:
            blob = torch.load(os.path.join(self.embeds_root, ann["vid"] + ".pt"), map_location="cpu", weights_only=True)
            for k in ("video_embeds", "audio_embeds"):
                if k in blob:
                    rec[k] = blob[k]
            rec["timestamps"] = [int(t) for t in blob["timestamps"]]
            return rec
        path = os.path.join(self.vis_root, ann["vid"] + ".mp4")
        if self.audio_processor is not None:
            rec["audio"] = self._call(self.audio_processor, path, ann)
        if getattr(self.video_processor, "device", None) is not None and hasattr(self.video_processor, "raw"):
            # a device processor: the record carries the decoded bytes and the clip's augmentation, the pixels are made on the GPU
            # inside the model (XInstructBLIP(video_processor=...)); no "video" key
            fn = self.video_processor.raw
            if "start" in ann and "clip" in inspect.signature(fn).parameters:
                frames, box, flip, indices, fps = fn(path, clip=(float(ann["start"]), float(ann["end"])))
            else:
                frames, box, flip, indices, fps = fn(path)
            rec["video_raw"], rec["video_box"], rec["video_flip"] = frames, box, torch.tensor(int(flip), dtype=torch.int64)
        else:
            video, indices, fps = self._call(self.video_processor, path, ann)
            rec["video"] = video
        rec["timestamps"] = [round(idx / fps) for idx in indices]
        return rec


class SyntheticMRDataset(Dataset):
    """Seeded stand-in corpus of pre-extracted features (no dataset exists offline): ``n`` videos of ``T``
    positions, one target window each; the target positions' features carry a common direction so a trained
    scorer has something to find.  ``queries_per_video = Q > 1`` (opt-in) gives every video ``Q`` annotation lines: record ``j`` is
    query ``j % Q`` of video ``j // Q``, with the video's features (those of ``Q = 1``, signal on the window of query 0) and a window of
    its own; query 0 is the record of ``Q = 1``."""

    def __init__(self, n: int = 8, T: int = 20, seed: int = 0, duration: int = 40, kv_video: int = 257, kv_audio: int = 256,
                 modalities=("video", "audio"), signal: float = 0.0, queries_per_video: int = 1):
        self.n, self.T, self.seed, self.duration = n, T, seed, duration
        self.kv = {"video": (kv_video, 1408), "audio": (kv_audio, 768)}
        self.modalities, self.signal = tuple(modalities), signal
        self.queries_per_video = max(1, int(queries_per_video))

    def __len__(self) -> int:
        return self.n * self.queries_per_video

    def _window(self, g: torch.Generator):
        s = int(torch.randint(0, self.T - 2, (1,), generator=g))
        return s, min(self.T - 1, s + 1 + int(torch.randint(1, max(2, self.T // 3), (1,), generator=g)))

    def _line(self, j: int):
        """(video i, query r, the video's generator after the draw of query 0's window, window of query 0, window of query r)."""
        i, r = divmod(j, self.queries_per_video)
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        w0 = self._window(g)
        wr = w0 if r == 0 else self._window(torch.Generator().manual_seed((self.seed * 100003 + i) * 131 + r))
        return i, r, g, w0, wr

    @property
    def annotation(self) -> List[dict]:
        """The annotation lines ``MRDataset`` would hold for this corpus (``queries_per_video`` lines per video), without the features."""
        out = []
        for j in range(len(self)):
            i, r, _, _, (s, e) = self._line(j)
            ts = [round(k * self.duration / self.T) for k in range(self.T)]
            out.append({"qid": j, "query": self._query(i, r), "vid": f"syn{i}", "duration": self.duration,
                        "relevant_windows": [[ts[s], ts[e]]]})
        return out

    @staticmethod
    def _query(i: int, r: int) -> str:
        return f"synthetic event number {i}" + (f", part {r}" if r else "")

    def __getitem__(self, j: int) -> Dict[str, object]:
        i, r, g, (s0, e0), (s, e) = self._line(j)
        step = self.duration / self.T
        ts = [round(k * step) for k in range(self.T)]
        rec: Dict[str, object] = {"text_input": build_prompt(self._query(i, r)), "text_output": str([[ts[s], ts[e]]]),
                                  "timestamps": ts, "duration": self.duration, "qid": j, "query": self._query(i, r), "vid": f"syn{i}"}
        for m in self.modalities:
            kv, width = self.kv[m]
            x = torch.randn(self.T, kv, width, generator=g)
            if self.signal:
                x[s0:e0 + 1] += self.signal * torch.randn(1, 1, width, generator=torch.Generator().manual_seed(self.seed + 7))
            rec[f"{m}_embeds"] = x
        return rec


def collate_fn(batch: List[dict]) -> Dict[str, object]:
    """``utils/mr_dataset.py:113-119``: tensors are stacked, everything else stays a list."""
    return {k: (torch.stack([b[k] for b in batch], dim=0) if isinstance(batch[0][k], torch.Tensor) else [b[k] for b in batch])
            for k in batch[0]}


# ---- several queries per video (XInstructBLIP.encode_fuse_multi) ------------------------------------------------
GROUPED_KEYS = ("qid", "query", "text_input", "text_output")


def group_by_video(annotation: Sequence[dict], max_queries: int = 16) -> List[List[int]]:
    """The annotation lines grouped by ``vid``: one list of line indices per video, videos in order of first appearance, lines in
    file order; a video with more than ``max_queries`` lines is cut into consecutive chunks of at most ``max_queries``."""
    if max_queries < 1:
        raise ValueError("max_queries must be >= 1")
    by_vid: Dict[object, List[int]] = {}
    for i, ann in enumerate(annotation):
        by_vid.setdefault(ann["vid"], []).append(i)
    return [idx[c: c + max_queries] for idx in by_vid.values() for c in range(0, len(idx), max_queries)]


def pad_queries(queries: Sequence[Sequence[object]]) -> Tuple[List[List[object]], List[int]]:
    """Ragged per-video lists -> (lists padded to the largest count by repeating each list's last entry, the original counts)."""
    counts = [len(q) for q in queries]
    if not counts or min(counts) < 1:
        raise ValueError("every video needs at least one query")
    width = max(counts)
    return [list(q) + [q[-1]] * (width - len(q)) for q in queries], counts


def drop_padding(rows: Sequence[Sequence[object]], counts: Sequence[int]) -> List[List[object]]:
    """Inverse of ``pad_queries`` on per-slot results: the first ``counts[b]`` entries of row ``b``."""
    return [list(r[:c]) for r, c in zip(rows, counts)]


def restore_order(groups: Sequence[Sequence[int]], results: Sequence[Sequence[object]]) -> List[object]:
    """Per-group results (``results[g][k]`` belongs to annotation line ``groups[g][k]``) back in the annotation file's order."""
    n = sum(len(g) for g in groups)
    out: List[object] = [None] * n
    seen = 0
    for g, r in zip(groups, results):
        if len(g) != len(r):
            raise ValueError(f"group of {len(g)} lines got {len(r)} results")
        for i, x in zip(g, r):
            out[i] = x
            seen += 1
    if seen != n or len(groups) != len(results):
        raise ValueError("results do not cover the groups")
    return out


def bpt_index(bs: int, num: int, prompts: int) -> torch.Tensor:
    """Gather index that brings rows ordered (video b, position t, prompt p) -- what ``forward_multi`` scores -- to (b, p, t), the
    order in which the scorer's span / window heads see ``bs * prompts`` videos of ``num`` positions: ``out[j] = rows[index[j]]``."""
    return torch.arange(bs * num * prompts).view(bs, num, prompts).permute(0, 2, 1).reshape(-1)


class VideoGroupedDataset(Dataset):
    """``base`` (an ``MRDataset``, or anything with its ``annotation`` list and records) regrouped so that one record is one video with
    up to ``max_queries`` of its queries: the video is loaded ONCE per group, ``qid`` / ``query`` / ``text_input`` / ``text_output``
    are lists, and ``index`` holds the annotation line numbers (``restore_order``)."""

    def __init__(self, base: Dataset, max_queries: int = 16):
        self.base, self.max_queries = base, int(max_queries)
        self.annotation = list(base.annotation)
        self.groups = group_by_video(self.annotation, self.max_queries)

    def __len__(self) -> int:
        return len(self.groups)

    def __getitem__(self, g: int) -> Dict[str, object]:
        idx = self.groups[g]
        rec = dict(self.base[idx[0]])
        anns = [self.annotation[i] for i in idx]
        rec["qid"] = [a["qid"] for a in anns]
        rec["query"] = [a["query"] for a in anns]
        rec["text_input"] = [build_prompt(a["query"]) for a in anns]
        rec["text_output"] = [str(a["relevant_windows"]) for a in anns]
        rec["index"] = list(idx)
        return rec


def collate_grouped(batch: List[dict]) -> Dict[str, object]:
    """``collate_fn`` for ``VideoGroupedDataset`` records: tensors are stacked, the per-query lists stay one list per video."""
    return collate_fn(batch)


def prepare_sample(samples: dict, device=None) -> dict:
    """What LAVIS ``prepare_sample(samples, cuda_enabled=True)`` does for the trainer (``utils/trainer.py:125``;
    third-party ``salesforce-lavis``, unpinned): move every tensor of the batch to the device."""
    if device is None:
        return samples
    return {k: (v.to(device, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in samples.items()}
