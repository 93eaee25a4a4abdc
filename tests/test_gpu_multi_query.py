"""Several prompts per clip over one shared K/V cache, on the GPU: the cross core (both ``multi_core`` forms, through
``mra_debug_shared_kv_attention`` = the forward's own launch code) against the float64 reference and derived bound of
``tests/multi_query_cases.py``; ``mra_qformer_forward_multi`` against the oracle and against ``forward_fused`` on replicated encoder rows;
the model-level ``encode_fuse_multi`` / ``generate_multi`` and ``evaluate --group-by-video``."""
import functools
import json

import pytest
import torch

import multi_query_cases as M
from oracle import qformer_ref as O
from test_gpu_parity import LOGIT_RTOL, Z_ATOL, build_qformer, oracle_cfg

pytestmark = pytest.mark.gpu

CORES = (0, 1)
HEADS = 2
# the grid split of long KV: both cores' rules (attn_pick_split / attn_shared_pick_split, csrc/attention.hip) start at 64 tiles; 65 tiles
# = kv 2049 is past it for both (core 0: 4 splits of 17 tiles; core 1: 33 two-tile stages in 4 splits of 9)
SPLIT_KV = 2049


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def run_core(q, k, v, P, core, dev):
    """q [N, heads, 32, 64], k / v [enc_items, heads, kv, 64] (CPU) -> ctx [N, heads, 32, 64] (CPU) through the debug entry."""
    from mraudio_amd import _lib

    L = _lib.lib()
    enc_items, heads, kv = k.shape[0], k.shape[1], k.shape[2]
    qd, kd, vd = M.pack_rows(q).to(dev), k.contiguous().to(dev), v.contiguous().to(dev)
    ctx = torch.full_like(qd, float("nan"))
    nbytes = int(L.mra_debug_shared_kv_workspace_bytes(enc_items, P, heads, kv, core))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.mra_debug_shared_kv_attention(_lib.ptr(qd), _lib.ptr(kd), _lib.ptr(vd), _lib.mra_dtype(q.dtype), enc_items, P, heads, kv, core,
                                                   _lib.ptr(ctx), _lib.ptr(ws), nbytes, _lib.current_stream()), "mra_debug_shared_kv_attention")
    torch.cuda.synchronize(dev)
    return M.unpack_rows(ctx.cpu(), heads), nbytes


@functools.lru_cache(maxsize=None)
def case(kind, enc_items, P, heads, kv, dtype):
    """Inputs and float64 reference of one case, computed once and shared by both cores."""
    q, k, v = M.make_multi(kind, enc_items, P, heads, kv, dtype)
    ref, bound = M.multi_ref(q, k, v, P)
    return q, k, v, ref, bound


# ---- 1. the core against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("kv", (1, 31, 32, 33, 257))
@pytest.mark.parametrize("P", (1, 3, 4, 5, 9))
def test_core_f16_every_family_inside_the_bound(P, kv, core, dev):
    for kind in M.families_for(kv):
        q, k, v, ref, bound = case(kind, 2, P, HEADS, kv, torch.float16)
        out, _ = run_core(q, k, v, P, core, dev)
        r = M.worst_ratio(out, ref, bound)
        print(f"core {core} P={P} kv={kv} {kind}: error / bound = {r:.3f}")
        assert r <= 1.0, (kind, P, kv, core, r)


@pytest.mark.parametrize("core", CORES)
@pytest.mark.parametrize("kv", (33, 257))
@pytest.mark.parametrize("P", (1, 3, 4, 5, 9))
def test_core_bf16_inside_the_bound(P, kv, core, dev):
    for kind in ("mild", "negative"):
        q, k, v, ref, bound = case(kind, 2, P, HEADS, kv, torch.bfloat16)
        out, _ = run_core(q, k, v, P, core, dev)
        r = M.worst_ratio(out, ref, bound)
        print(f"core {core} bf16 P={P} kv={kv} {kind}: error / bound = {r:.3f}")
        assert r <= 1.0, (kind, P, kv, core, r)


@pytest.mark.parametrize("core", CORES)
def test_core_past_the_kv_split_threshold(core, dev):
    for kind in ("mild", "peaked", "negative", f"onehot@{SPLIT_KV - 1}"):
        q, k, v, ref, bound = case(kind, 1, 5, 1, SPLIT_KV, torch.float16)
        out, nbytes = run_core(q, k, v, 5, core, dev)
        assert nbytes > 0, "this shape must take the grid-split path (partials in the workspace)"
        r = M.worst_ratio(out, ref, bound)
        print(f"core {core} split kv={SPLIT_KV} {kind}: error / bound = {r:.3f}")
        assert r <= 1.0, (kind, core, r)


# ---- 2. no cross-talk between prompt slots -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("core", CORES)
def test_permuting_the_prompt_slots_permutes_the_context_bit_for_bit(core, dev):
    P, kv = 5, 257
    q, k, v, _, _ = case("mild", 2, P, HEADS, kv, torch.float16)
    out, _ = run_core(q, k, v, P, core, dev)
    perm = torch.tensor([3, 0, 4, 2, 1])
    rows = torch.cat([i * P + perm for i in range(2)])
    out_p, _ = run_core(q[rows], k, v, P, core, dev)
    assert torch.equal(out_p, out[rows])


# ---- 3 - 5. the forward -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def video(dev):
    qf, cfg = build_qformer(dev, 1408, seed=0)
    return qf, cfg, O.init_weights(oracle_cfg(cfg), seed=0, perturb=True)


@pytest.fixture(scope="module")
def audio(dev):
    qf, cfg = build_qformer(dev, 768, seed=1)
    return qf, cfg, O.init_weights(oracle_cfg(cfg), seed=1, perturb=True)


def make_rows(cfg, rows, L, seed, ragged=True):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, cfg.vocab, (rows, L), generator=g)
    tmask = torch.ones(rows, L, dtype=torch.long)
    if ragged:
        for r in range(rows):   # a different number of padding columns per row, so the masks differ between the prompt slots of an item
            tmask[r, L - (r % 4):] = 0
    att = torch.cat([torch.ones(rows, cfg.n_query, dtype=torch.long), tmask], 1)
    return ids, att


def test_one_prompt_is_the_kv_cache_forward(video, dev):
    qf, cfg, _ = video
    n, kv, L = 4, 257, 9
    g = torch.Generator().manual_seed(5)
    enc = qf.modality_ln(torch.randn(n, kv, cfg.enc_width, generator=g).to(dev))
    ids, att = make_rows(cfg, n, L, 6)
    qf.set_cross_mode("kv_cache")
    try:
        ref = qf.forward_fused(ids.to(dev), att.to(dev), enc, want_query=True, want_cls=True)
    finally:
        qf.set_cross_mode("auto")
    for core in CORES:
        qf.set_option("multi_core", core)
        got = qf.forward_multi(ids.to(dev), att.to(dev), enc, 1, want_query=True, want_cls=True)
        assert torch.equal(got["query"], ref["query"]) and torch.equal(got["cls"], ref["cls"])
    qf.set_option("multi_core", 0)


@pytest.mark.parametrize("which", ["video", "audio"])
def test_forward_multi_against_the_oracle_and_the_replicated_forward(which, video, audio, dev):
    qf, cfg, w = video if which == "video" else audio
    ocfg = oracle_cfg(cfg)
    n, P, L, kv = 2, 3, 9, 257 if which == "video" else 256
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(n, kv, cfg.enc_width, generator=g)
    ids, att = make_rows(cfg, n * P, L, 12)
    assert not torch.equal(att[0], att[1])
    enc = qf.modality_ln(feats.to(dev))
    enc_ref = O.modality_layernorm(feats, w["ln.weight"], w["ln.bias"]).repeat_interleave(P, 0)
    h = O.qformer_forward(w, ocfg, ids, att, w["query_tokens"].expand(n * P, -1, -1), enc_ref)
    rep = qf.forward_fused(ids.to(dev), att.to(dev), enc.repeat_interleave(P, 0), want_query=True, want_cls=True)
    try:
        for core in CORES:
            qf.set_option("multi_core", core)
            got = qf.forward_multi(ids.to(dev), att.to(dev), enc, P, want_query=True, want_cls=True)
            for name, ref in (("query", h[:, :32]), ("cls", h[:, 32])):
                x = got[name].cpu()
                d, rel = (x - ref).abs().max().item(), ((x - ref).norm() / ref.norm()).item()
                d2, rel2 = (x - rep[name].cpu()).abs().max().item(), ((x - rep[name].cpu()).norm() / ref.norm()).item()
                print(f"{which} core {core} {name}: vs oracle max|d| {d:.2e} rel {rel:.2e}; vs replicated forward max|d| {d2:.2e} rel {rel2:.2e}")
                assert d < Z_ATOL and rel < 2e-3, (which, core, name, d, rel)
                assert d2 < 2 * Z_ATOL and rel2 < 2 * 2e-3, (which, core, name, d2, rel2)
    finally:
        qf.set_option("multi_core", 0)


def test_the_cache_is_shared_in_the_workspace(video):
    from mraudio_amd import _lib

    qf, _, _ = video
    L = _lib.lib()
    n, P, Lt, kv = 2, 4, 9, 257
    qf.set_cross_mode("kv_cache")
    try:
        replicated = int(L.mra_qformer_workspace_bytes(qf._handle, n * P, Lt, kv))
    finally:
        qf.set_cross_mode("auto")
    cache = int(L.mra_kv_cache_bytes(qf._handle, n, kv))
    for core in CORES:
        qf.set_option("multi_core", core)
        shared = int(L.mra_qformer_multi_workspace_bytes(qf._handle, n, P, Lt, kv))
        assert shared > 0 and replicated - shared >= (P - 1) * cache - 64 * 1024, (core, replicated, shared, cache)
    qf.set_option("multi_core", 0)


# ---- 6 - 7. the model ---------------------------------------------------------------------------------------------------------------
PROMPTS = [["Query: a person opens the door.\nRelevant windows: ", "Query: someone is cooking in the kitchen while music plays.\nRelevant windows: ",
            "Query: a dog barks.\nRelevant windows: "], ["Query: the crowd applauds after the speech ends.\nRelevant windows: "]]


def model_samples():
    g = torch.Generator().manual_seed(23)
    bs, num = 2, 4
    return {"video_embeds": torch.randn(bs, num, 257, 1408, generator=g), "audio_embeds": torch.randn(bs, num, 256, 768, generator=g),
            "timestamps": [[0, 3, 6, 9], [1, 4, 8, 12]], "duration": [12, 14]}


def one_video(samples, b, prompt):
    return {"video_embeds": samples["video_embeds"][b:b + 1], "audio_embeds": samples["audio_embeds"][b:b + 1],
            "timestamps": [samples["timestamps"][b]], "duration": [samples["duration"][b]], "text_input": [prompt]}


def check_model_against_single_calls(model, samples, out):
    from mraudio_amd import scorer

    assert [int(f.shape[0]) for f in out["fused"]] == [3, 1] and out["counts"] == [3, 1]     # the padded slots of video 1 are absent
    assert all(tuple(f.shape) == (c, 4) for f, c in zip(out["fused"], (3, 1)))
    worst = 0.0
    for b, qs in enumerate(PROMPTS):
        for p, prompt in enumerate(qs):
            ref = model.encode_fuse(one_video(samples, b, prompt))["fused"]
            d, scale = (out["fused"][b][p] - ref).abs().max().item(), ref.abs().max().item()
            worst = max(worst, d / scale)
            assert d <= 2 * LOGIT_RTOL * scale, (b, p, d, scale)
    print(f"fused logits vs one encode_fuse per (video, query): worst |d| / max|logit| = {worst:.2e} (bar {2 * LOGIT_RTOL:.0e})")
    for b, f in enumerate(out["fused"]):
        c = int(f.shape[0])
        assert torch.equal(out["spans"][b], scorer.spans_from_logits(f.reshape(-1), c, 4, model.score_alpha))
        win, sc, cnt = scorer.windows_from_logits(f.reshape(-1), c, 4, model.score_alpha, model.top_k, model.nms_thd, model.max_window)
        assert torch.equal(out["windows"][b], win) and torch.equal(out["window_scores"][b], sc) and torch.equal(out["window_counts"][b], cnt)
    assert set(out["logit"]) == {"video", "audio"} and [tuple(x.shape) for x in out["logit"]["video"]] == [(3, 4), (1, 4)]


def test_model_multi_query_against_one_call_per_video_and_query(dev):
    from mraudio_amd.models.xinstructblip import XInstructBLIP
    from mraudio_amd.utils.spans import moment_str_to_list, post_process

    model = XInstructBLIP(seed=0, perturb=True, device=dev, compat_repeat=False, top_k=3)
    samples = model_samples()
    for core in CORES:
        for m in model.modalities:
            getattr(model, f"{m}_Qformer").set_option("multi_core", core)
        check_model_against_single_calls(model, samples, model.encode_fuse_multi(samples, PROMPTS))
    # one stream or one per modality: the same launches, so the same bits
    assert model.overlap_modalities
    forked = model.encode_fuse_multi(samples, PROMPTS)
    model.overlap_modalities = False
    plain = model.encode_fuse_multi(samples, PROMPTS)
    model.overlap_modalities = True
    for key in ("fused", "spans", "windows", "window_scores", "window_counts"):
        assert all(torch.equal(a, b) for a, b in zip(forked[key], plain[key])), key
    assert all(torch.equal(a, b) for m in model.modalities for a, b in zip(forked["logit"][m], plain["logit"][m]))
    strings = model.generate_multi(samples, PROMPTS)
    assert [len(s) for s in strings] == [3, 1]
    for row in strings:
        for s in row:
            assert isinstance(s, str) and len(moment_str_to_list(post_process(s))[0]) == 2
    texts, records, sal = model.generate_multi_windows(samples, PROMPTS)
    assert [len(t) for t in texts] == [3, 1] and [len(r) for r in records] == [3, 1] and [len(x) for x in sal] == [3, 1]
    # one query per video for the whole call is encode_fuse itself
    single = model.encode_fuse_multi(samples, [[PROMPTS[0][0]], [PROMPTS[1][0]]])
    both = dict(samples, text_input=[PROMPTS[0][0], PROMPTS[1][0]])
    assert torch.equal(torch.stack([f[0] for f in single["fused"]]).reshape(-1), model.encode_fuse(both)["fused"])


class _TwoRanks:
    def size(self):
        return 2


def test_split_precision_and_process_groups(video, dev):
    from mraudio_amd import MraError, _lib
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    # the ABI entry refuses split precision
    qf, cfg, _ = video
    g = torch.Generator().manual_seed(5)
    enc = qf.modality_ln(torch.randn(2, 257, cfg.enc_width, generator=g).to(dev))
    ids, att = make_rows(cfg, 4, 9, 6)
    qf.set_cross_precision("split")
    try:
        q = torch.empty(4, 32, cfg.hidden, device=dev)
        ws = torch.empty(int(_lib.lib().mra_qformer_multi_workspace_bytes(qf._handle, 2, 2, 9, 257)) + 256, dtype=torch.uint8, device=dev)
        rc = _lib.lib().mra_qformer_forward_multi(qf._handle, _lib.ptr(ids.to(dev)), _lib.ptr(att.to(dev)), _lib.ptr(enc), 2, 2, 9, 257, _lib.ptr(q), None,
                                                  _lib.ptr(ws), ws.numel(), _lib.current_stream())
        assert rc == -2   # MRA_ESTATE
        with pytest.raises(MraError):
            qf.forward_multi(ids.to(dev), att.to(dev), enc, 2)
    finally:
        qf.set_cross_precision("op")
    # the model falls back to one ordinary forward per prompt slot, inside the same bar
    model = XInstructBLIP(seed=0, perturb=True, device=dev, compat_repeat=False, top_k=3, cross_precision="split")
    samples = model_samples()
    check_model_against_single_calls(model, samples, model.encode_fuse_multi(samples, PROMPTS))
    # the multi path is not sharded
    model.process_group = _TwoRanks()
    with pytest.raises(MraError):
        model.encode_fuse_multi(samples, PROMPTS)


# ---- 8. evaluate --group-by-video ---------------------------------------------------------------------------------------------------
def test_evaluate_group_by_video_writes_one_record_per_query_in_annotation_order(dev, tmp_path):
    from torch.utils.data import DataLoader

    from mraudio_amd.evaluate import run_inference_grouped
    from mraudio_amd.models.xinstructblip import XInstructBLIP
    from mraudio_amd.utils.mr_dataset import SyntheticMRDataset, VideoGroupedDataset, collate_grouped

    class TwoQueriesEach(SyntheticMRDataset):
        """4 annotation lines over 2 synthetic videos, interleaved: lines 0 and 2 ask video 0, lines 1 and 3 video 1."""

        @property
        def annotation(self):
            base = SyntheticMRDataset.annotation.fget(self)
            return [dict(base[i % 2], qid=100 + i, query=f"{base[i % 2]['query']} take {i // 2}") for i in range(4)]

        def __len__(self):
            return 4

        def __getitem__(self, i):
            a = self.annotation[i]
            return dict(SyntheticMRDataset.__getitem__(self, i % 2), qid=a["qid"], query=a["query"])

    ds = TwoQueriesEach(2, T=4)
    grouped = VideoGroupedDataset(ds, max_queries=16)
    assert grouped.groups == [[0, 2], [1, 3]]
    model = XInstructBLIP(seed=0, perturb=True, device=dev)
    out = tmp_path / "pred.jsonl"
    recs = run_inference_grouped(model, DataLoader(grouped, shuffle=False, batch_size=2, collate_fn=collate_grouped), str(out), device=dev)
    lines = [json.loads(x) for x in out.read_text().splitlines()]
    assert lines == json.loads(json.dumps(recs)) and [r["qid"] for r in lines] == [100, 101, 102, 103]
    assert [r["vid"] for r in lines] == ["syn0", "syn1", "syn0", "syn1"]
    for r in lines:
        assert set(r) == {"qid", "query", "vid", "pred_relevant_windows", "raw_out", "pred_saliency_scores"}
        assert len(r["pred_saliency_scores"]) == 4 and len(r["pred_relevant_windows"][0]) == 2


def test_evaluate_cli_group_by_video(tmp_path, capsys):
    from mraudio_amd.evaluate import main

    plain, grouped = tmp_path / "plain.jsonl", tmp_path / "grouped.jsonl"
    main(["--synthetic", "4", "--output-file", str(plain)])
    main(["--synthetic", "4", "--group-by-video", "--max-queries-per-call", "2", "--output-file", str(grouped)])
    a = [json.loads(x) for x in plain.read_text().splitlines()]
    b = [json.loads(x) for x in grouped.read_text().splitlines()]
    assert [r["qid"] for r in b] == [0, 1, 2, 3] and [set(r) for r in a] == [set(r) for r in b]
    # one query per video: the grouped run is the plain path with aligned prompts (the plain run pairs prompts as the reference does)
    assert [(r["qid"], r["query"], r["vid"]) for r in a] == [(r["qid"], r["query"], r["vid"]) for r in b]
