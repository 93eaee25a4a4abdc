"""Ranked-window head without a GPU: the definition's host reference (hand cases, invariants, sensitivity to three wrong
rules), what the ranked list buys in MR-mAP, the text / record / evaluate plumbing and the ABI's argument checks."""
import ctypes
import json

import numpy as np
import pytest

import window_cases as W
from mraudio_amd import _lib, scorer
from mraudio_amd.eval.mr_eval import compute_mr_ap
from mraudio_amd.utils.spans import moment_str_to_list, post_process

HAND = [0, 1, 1, 0, 0, .75, .75, 0]
S = 2 ** 20


def picks(x, **kw):
    kw.setdefault("top_k", 5)
    return [(s, e, sc / S) for s, e, sc in W.windows_ref_one(np.asarray(x, dtype=np.float32), **kw)]


def test_hand_cases():
    assert picks(HAND, nms_thd=0.25) == [(1, 2, 1.0), (5, 6, 0.5)]
    assert picks(HAND, nms_thd=0.5) == [(1, 2, 1.0), (1, 1, .5), (2, 2, .5), (5, 6, .5), (1, 6, .5)]
    assert picks(HAND, nms_thd=0.5, max_len=1) == [(1, 1, .5), (2, 2, .5), (5, 5, .25), (6, 6, .25)]
    assert picks([.3] * 6) == [(0, 0, 0.0)]
    assert picks([2.5]) == [(0, 0, 0.0)]
    assert picks([0, 1], alpha=0.0, nms_thd=0.5) == [(1, 1, 1.0), (0, 1, 1.0)]


def test_array_outputs_fill_unused_slots():
    win, sc, cnt = W.windows_ref(np.asarray([HAND, [.3] * 8], dtype=np.float32), 2, 8, top_k=4, nms_thd=0.25)
    assert win.dtype == np.int32 and sc.dtype == np.float32 and cnt.dtype == np.int32
    assert cnt.tolist() == [2, 1]
    assert win[0].tolist() == [[1, 2], [5, 6], [-1, -1], [-1, -1]] and sc[0].tolist() == [1.0, 0.5, 0.0, 0.0]
    assert win[1].tolist() == [[0, 0], [-1, -1], [-1, -1], [-1, -1]] and sc[1].tolist() == [0.0] * 4


@pytest.mark.parametrize("family", W.FAMILIES)
@pytest.mark.parametrize("T", [1, 2, 3, 8, 63, 65, 129])
def test_invariants(family, T):
    for seed, (nms_thd, top_k, alpha) in enumerate([(0.25, 8, 0.5), (0.0, 3, 0.5), (0.9, 8, 0.0)]):
        x = W.make_batch(family, T, 2, seed)
        win, sc, cnt = W.windows_ref(x, 2, T, alpha=alpha, top_k=top_k, nms_thd=nms_thd)
        for v in range(2):
            n = int(cnt[v])
            assert 1 <= n <= top_k
            assert (win[v, n:] == -1).all() and (sc[v, n:] == 0).all()
            w = win[v, :n].tolist()
            assert all(0 <= s <= e < T for s, e in w)
            assert all(sc[v, k] >= sc[v, k + 1] for k in range(n - 1))           # non-increasing
            assert sc[v, 0] >= 0 and all(sc[v, k] > 0 for k in range(1, n))
            for a in range(n):
                for b in range(a):
                    inter = max(0, min(w[a][1], w[b][1]) - max(w[a][0], w[b][0]) + 1)
                    union = (w[a][1] - w[a][0] + 1) + (w[b][1] - w[b][0] + 1) - inter
                    assert not float(inter) > float(np.float32(nms_thd)) * float(union)
            s, e, score = W.kadane_best(x[v], alpha)
            assert w[0] == [s, e] and sc[v, 0] == np.float32(score * 2.0 ** -20)   # rank 1: a maximum-sum window, tie rule included


@pytest.mark.parametrize("variant", ["long_tie", "exclusive_iou", "ge_suppress"])
def test_cases_see_the_wrong_variants(variant):
    """The inputs must tell each wrong rule from the right one: 72 inputs per family (6 lengths x 3 thresholds x 4 seeds), the variant has
    to differ on at least one of them.  Continuous families rarely tie, so the tie rule is seen mostly by ``quant``; the per-family counts
    are printed."""
    seen = 0
    for family in ("normal", "quant", "two_peak"):
        diff = total = 0
        for T in (2, 3, 8, 63, 65, 129):
            for nms_thd in (0.0, 0.5, 0.9):
                for seed in range(4):
                    x = W.make_logits(family, T, seed)
                    total += 1
                    diff += W.windows_ref_one(x, top_k=8, nms_thd=nms_thd) != W.windows_ref_one(x, top_k=8, nms_thd=nms_thd, variant=variant)
        print(f"{variant} on {family}: {diff}/{total} inputs differ")
        assert total == 72
        seen += diff
    assert seen >= 1


def map_fixture(n=40, T=60, seed=0):
    """40 queries of 60 clips with two disjoint ground-truth windows each: plateaus of height 1 and 0.8 plus noise 0.05."""
    rng = np.random.default_rng(seed)
    xs, gts = [], []
    for _ in range(n):
        la, lb = (int(v) for v in rng.integers(4, 10, size=2))
        a = int(rng.integers(0, T // 2 - la))
        b = int(rng.integers(T // 2 + 2, T - lb))
        x = rng.normal(0.0, 0.05, T)
        x[a:a + la] += 1.0
        x[b:b + lb] += 0.8
        xs.append(x.astype(np.float32))
        gts.append([[a, a + la - 1], [b, b + lb - 1]])
    return xs, gts


def seconds(s, e, clip=2):
    return [clip * s, clip * (e + 1)]


def test_ranked_list_lifts_mr_map():
    xs, gts = map_fixture()
    gt = [{"qid": i, "relevant_windows": [seconds(*w) for w in g]} for i, g in enumerate(gts)]
    top5, top1 = [], []
    for i, x in enumerate(xs):
        wins = [seconds(s, e) + [sc / S] for s, e, sc in W.windows_ref_one(x, alpha=0.5, top_k=5, nms_thd=0.25)]
        top5.append({"qid": i, "pred_relevant_windows": wins})
        top1.append({"qid": i, "pred_relevant_windows": wins[:1]})
    m5, m1 = compute_mr_ap(top5, gt)["average"], compute_mr_ap(top1, gt)["average"]
    print(f"MR-mAP average: top-5 {m5}, rank 1 alone {m1}")
    assert m1 <= 50.0      # one window cannot cover two ground-truth windows
    assert m5 > m1


def test_text_and_records_round_trip():
    x = np.asarray([HAND, HAND[::-1]], dtype=np.float32)
    win, sc, cnt = W.windows_ref(x, 2, 8, top_k=5, nms_thd=0.5)
    ts = [[3 * k for k in range(8)], [2 * k + 1 for k in range(8)]]
    texts = scorer.windows_to_text(win, cnt, ts)
    recs = scorer.windows_to_records(win, sc, cnt, ts)
    assert texts[0] == "[[3, 6], [3, 3], [6, 6], [15, 18], [3, 18]]"
    for v in range(2):
        pairs = [[ts[v][s], ts[v][e]] for s, e in win[v, :cnt[v]].tolist()]
        assert moment_str_to_list(post_process(texts[v])) == pairs
        assert [r[:2] for r in recs[v]] == pairs
        assert [r[2] for r in recs[v]] == [float(z) for z in sc[v, :cnt[v]]]
        assert all(isinstance(r[0], int) and isinstance(r[2], float) for r in recs[v])
    import torch
    assert scorer.windows_to_text(torch.from_numpy(win), torch.from_numpy(cnt), ts) == texts
    assert scorer.windows_to_records(torch.from_numpy(win), torch.from_numpy(sc), torch.from_numpy(cnt), ts) == recs


class FakeModel:
    def __init__(self):
        self.calls = []

    def generate_windows(self, samples):
        self.calls.append("windows")
        n = len(samples["qid"])
        return ["[[4, 8], [0, 2]]"] * n, [[[4, 8, 1.5], [0, 2, 0.25]] for _ in range(n)], [[0.1, 0.9, 0.2]] * n

    def generate_with_scores(self, samples):
        self.calls.append("scores")
        return ["[[4, 8]]"] * len(samples["qid"]), [[0.1, 0.9, 0.2]] * len(samples["qid"])


def test_run_inference_writes_ranked_triples(tmp_path):
    from mraudio_amd.evaluate import run_inference

    batches = [{"qid": [0, 1], "query": ["a", "b"], "vid": ["v0", "v1"]}, {"qid": [2], "query": ["c"], "vid": ["v2"]}]
    model = FakeModel()
    out = tmp_path / "ranked.jsonl"
    recs = run_inference(model, batches, str(out), top_k=5)
    lines = [json.loads(x) for x in out.read_text().splitlines()]
    assert lines == recs and len(lines) == 3 and model.calls == ["windows", "windows"]
    for r in lines:
        assert r["pred_relevant_windows"] == [[4, 8, 1.5], [0, 2, 0.25]]          # rank order kept, scores attached
        assert r["raw_out"] == "[[4, 8], [0, 2]]" and r["pred_saliency_scores"] == [0.1, 0.9, 0.2]
    assert compute_mr_ap(lines, [{"qid": q, "relevant_windows": [[0, 2], [4, 8]]} for q in range(3)])["average"] == 100.0
    # top_k == 1: the path and the file of before
    model = FakeModel()
    one = tmp_path / "one.jsonl"
    run_inference(model, batches, str(one), top_k=1)
    old = tmp_path / "old.jsonl"
    run_inference(FakeModel(), batches, str(old))
    assert model.calls == ["scores", "scores"] and one.read_bytes() == old.read_bytes()
    assert json.loads(one.read_text().splitlines()[0])["pred_relevant_windows"] == [[4, 8]]


def test_parser_flags():
    from mraudio_amd.evaluate import build_parser

    a = build_parser().parse_args(["--output-file", "x"])
    assert (a.top_k, a.nms_thd, a.max_window) == (1, 0.25, 0)
    a = build_parser().parse_args(["--output-file", "x", "--top-k", "5", "--nms-thd", "0.5", "--max-window", "12"])
    assert (a.top_k, a.nms_thd, a.max_window) == (5, 0.5, 12)


def test_abi_rejects_bad_arguments_before_touching_the_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(4096)        # host memory: never dereferenced, every call below returns before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(logits=p, videos=1, clips=8, alpha=0.5, top_k=5, nms_thd=0.25, max_len=0, windows=p, scores=p, counts=p):
        return lib.mra_windows_from_logits(logits, videos, clips, alpha, top_k, nms_thd, max_len, windows, scores, counts, None)

    assert call(logits=None, videos=0, windows=None, scores=None, counts=None) == 0    # empty input is a no-op
    bad = [(dict(videos=-1), b"videos"), (dict(logits=None), b"null"), (dict(windows=None), b"null"), (dict(scores=None), b"null"),
           (dict(counts=None), b"null"), (dict(clips=0), b"clips"), (dict(clips=4097), b"clips"), (dict(top_k=0), b"top_k"),
           (dict(top_k=65), b"top_k"), (dict(nms_thd=-0.25), b"nms_thd"), (dict(nms_thd=1.0), b"nms_thd"),
           (dict(nms_thd=float("nan")), b"nms_thd"), (dict(max_len=-1), b"max_len")]
    for kw, word in bad:
        assert lib.mra_cosine_score(None, None, 1, -1, 32, 768, None, None, None) == -1     # leaves another message behind
        assert call(**kw) == -1, kw
        assert word in lib.mra_last_error(), (kw, lib.mra_last_error())
