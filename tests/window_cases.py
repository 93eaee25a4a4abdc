"""Host reference and seeded inputs for the ranked-window head (``mra_windows_from_logits``, ``include/mra.h``).

``windows_ref`` is the definition by brute force: enumerate every window, sort by the key, walk the sorted list with
greedy NMS.  It shares no step with the kernel's repeated argmax over cached per-start maxima.  Scores are exact
integers (int64 holds them: |q| <= 2^41, at most 4096 terms), so the order does not depend on the platform.
"""
from __future__ import annotations

import numpy as np

FAMILIES = ("normal", "quant", "two_peak", "ramp", "constant", "large", "tiny")
SCALE = float(2 ** 20)
CLAMP = float(2 ** 40)


def make_logits(family: str, T: int, seed: int = 0) -> np.ndarray:
    """One video's fp32 logits ``[T]``; the same (family, T, seed) always gives the same values."""
    rng = np.random.default_rng([FAMILIES.index(family), T, seed])
    if family == "normal":
        x = rng.standard_normal(T)
    elif family == "quant":       # four levels: many exact score ties
        x = rng.choice(np.array([0.0, 0.25, 0.5, 1.0]), size=T)
    elif family == "two_peak":    # plateaus at 1 and 0.9 plus noise
        x = rng.normal(0.0, 0.05, T)
        a, b = sorted(rng.choice(T, size=2, replace=False).tolist()) if T >= 2 else (0, 0)
        w = max(1, T // 6)
        x[a:a + w] += 1.0
        x[b:b + w] += 0.9
    elif family == "ramp":
        x = np.arange(T, dtype=np.float64) / max(T - 1, 1) * (1.0 if seed % 2 == 0 else -1.0) + 0.125 * seed
    elif family == "constant":
        x = np.full(T, 0.3 + 0.1 * seed)
    elif family == "large":
        x = rng.standard_normal(T) * 1000.0
    elif family == "tiny":        # steps of 1e-8 around 0.5: distinct floats that collapse to ties after quantisation
        x = 0.5 + rng.integers(-8, 9, size=T) * 1e-8
    else:
        raise ValueError(family)
    return np.asarray(x, dtype=np.float32)


def make_batch(family: str, T: int, videos: int, seed: int = 0) -> np.ndarray:
    """``[videos, T]`` with different content per video."""
    return np.stack([make_logits(family, T, seed * 1000 + v) for v in range(videos)])


def _fixed(x) -> np.ndarray:
    v = np.clip(np.asarray(x, dtype=np.float32).astype(np.float64) * SCALE, -CLAMP, CLAMP)
    return np.rint(v).astype(np.int64)


def prefix_sums(x: np.ndarray, alpha: float, contract: bool = False) -> np.ndarray:
    """Steps 1-3 of the definition: fp32 threshold (two roundings), 2^20 fixed point, exact int64 prefix sums."""
    x = np.asarray(x, dtype=np.float32)
    hi, lo = np.float32(x.max()), np.float32(x.min())
    if contract:   # the fma-contracted threshold, for the sensitivity study only
        thr = np.float32(np.float64(lo) + np.float64(np.float32(alpha)) * np.float64(np.float32(hi - lo)))
    else:
        prod = np.float32(np.float32(alpha) * np.float32(hi - lo))
        thr = np.float32(lo + prod)
    q = _fixed(x) - _fixed(thr)
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(q, dtype=np.int64)])


def windows_ref_one(x, alpha=0.5, top_k=10, nms_thd=0.25, max_len=0, variant: str = ""):
    """One video: ``[(s, e, score_int), ...]`` in rank order.  ``variant`` selects a deliberately wrong rule
    (``"long_tie"``, ``"exclusive_iou"``, ``"ge_suppress"``, ``"fma_thr"``) for the sensitivity tests."""
    x = np.asarray(x, dtype=np.float32)
    T = int(x.shape[0])
    P = prefix_sums(x, alpha, contract=variant == "fma_thr")
    cap = T if max_len == 0 else min(int(max_len), T)
    per_start = np.minimum(cap, T - np.arange(T))                      # windows of each start
    s = np.repeat(np.arange(T), per_start)
    e = s + np.arange(len(s)) - np.repeat(np.cumsum(per_start) - per_start, per_start)
    score = P[e + 1] - P[s]
    length = e - s + 1
    order = np.lexsort((s, -length if variant == "long_tie" else length, -score))   # last key is the primary one
    s, e, score, length = s[order], e[order], score[order], length[order]
    thd = np.float64(np.float32(nms_thd))
    alive = np.ones(len(s), dtype=bool)
    out = []
    plus = 0 if variant == "exclusive_iou" else 1
    while len(out) < top_k:
        idx = int(np.argmax(alive))
        if not alive[idx]:
            break
        if out and score[idx] <= 0:
            break
        ps, pe = int(s[idx]), int(e[idx])
        out.append((ps, pe, int(score[idx])))
        inter = np.maximum(0, np.minimum(e, pe) - np.maximum(s, ps) + plus).astype(np.float64)
        union = (length - 1 + plus) + (pe - ps + plus) - inter
        sup = inter >= thd * union if variant == "ge_suppress" else inter > thd * union
        alive &= ~sup
        alive[idx] = False   # holds by the rule itself (nms_thd < 1); kept so that the wrong variants terminate too
    return out


def windows_ref(logits, videos, clips, alpha=0.5, top_k=10, nms_thd=0.25, max_len=0, variant: str = ""):
    """The three outputs of ``mra_windows_from_logits`` as numpy arrays: windows int32 ``[V, top_k, 2]`` (unused -1),
    scores fp32 ``[V, top_k]`` (unused 0), counts int32 ``[V]``."""
    x = np.asarray(logits, dtype=np.float32).reshape(videos, clips)
    windows = np.full((videos, top_k, 2), -1, dtype=np.int32)
    scores = np.zeros((videos, top_k), dtype=np.float32)
    counts = np.zeros(videos, dtype=np.int32)
    for v in range(videos):
        picks = windows_ref_one(x[v], alpha, top_k, nms_thd, max_len, variant)
        counts[v] = len(picks)
        for k, (s, e, sc) in enumerate(picks):
            windows[v, k] = (s, e)
            scores[v, k] = np.float32(np.float64(sc) * 2.0 ** -20)
    return windows, scores, counts


def kadane_best(x, alpha=0.5):
    """Maximum-sum window under the tie rule (higher score, shorter, smaller start) in one pass: for every end the best
    start is the LAST minimum of the prefix sums so far (shortest window of that score)."""
    P = prefix_sums(x, alpha)
    best = None
    min_p, min_s = None, 0
    for e in range(len(P) - 1):
        if min_p is None or P[e] <= min_p:
            min_p, min_s = int(P[e]), e
        key = (-(int(P[e + 1]) - min_p), e - min_s + 1, min_s)
        if best is None or key < best[0]:
            best = (key, (min_s, e, int(P[e + 1]) - min_p))
    return best[1]

