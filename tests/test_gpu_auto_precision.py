"""``-m gpu``: the automatic cross-attention precision (``QFormer.set_cross_precision("auto")``, mra_qformer_set_cross_precision 2).

The first forward after a weight upload measures the median softmax row maximum of every cross layer (a histogram filled by the probe
variant of the row-factor kernel) and resolves to ``split`` iff the largest median reaches 0.5, to ``op`` otherwise.  Checked here:
the measured medians against the oracle's own probabilities, bit equality with explicit ``op`` where it resolves to op, the 1e-3
similarity-logit bar on the peaked fixtures of ``tests/test_gpu_headline.py`` (the f16 chain misses it from gain 5 on), re-probing
after every weight upload, the K/V-cache mode and short Kv, the pair forward's refusal and ``XInstructBLIP(cross_precision="auto")``.
"""
import ctypes as C

import pytest
import torch

from oracle import qformer_ref as O

pytestmark = pytest.mark.gpu

LOGIT_RTOL = 1e-3
MRA_ESTATE = -2                  # include/mra.h
MEDIAN_TOL = 1.0 / 256 + 0.02    # histogram bin width + what the f16 score chain may move a row maximum
PEAKED_CASES = [(2100, 4.0), (300, 4.0), (300, 5.0), (2100, 5.0), (2100, 7.0)]
_CASES = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _peaked_weights(cfg, seed, gain):
    """Seeded weights whose cross-attention query / key projections are scaled by ``gain`` each (scores x gain^2); the construction of
    the peaked fixture in tests/test_gpu_headline.py."""
    w = O.init_weights(cfg, seed=seed, perturb=True)
    for i in cfg.cross_layers():
        for nme in ("query", "key"):
            for part in ("weight", "bias"):
                k = f"bert.encoder.layer.{i}.crossattention.self.{nme}.{part}"
                w[k] = w[k] * gain
    return w


def _cross_probabilities(w, cfg, collect, enc, layer):
    """Attention probabilities of cross layer ``layer`` as the oracle computes them (from its collected states)."""
    p = f"bert.encoder.layer.{layer}."
    hq = collect[f"layer{layer}.attn"][:, :32]
    q = hq @ w[p + "crossattention.self.query.weight"].T + w[p + "crossattention.self.query.bias"]
    k = enc @ w[p + "crossattention.self.key.weight"].T + w[p + "crossattention.self.key.bias"]
    n = q.shape[0]
    q = q.view(n, 32, cfg.heads, 64).permute(0, 2, 1, 3)
    k = k.view(n, -1, cfg.heads, 64).permute(0, 2, 1, 3)
    return torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1)


def _qformer(dev, w, precision="op", cross_mode="auto"):
    from mraudio_amd.qformer import QFormer, QFormerConfig

    qf = QFormer(QFormerConfig(enc_width=1408), device=dev)
    _load(qf, w)
    qf.set_cross_mode(cross_mode)
    qf.set_cross_precision(precision)
    return qf


def _load(qf, w):
    qf.load_state_dict({k: v for k, v in w.items() if k.startswith("bert.")})
    for k in ("query_tokens", "ln.weight", "ln.bias"):
        qf.push(k, w[k])


def _case(dev, kv, gain):
    """Weights (gain None: the plain seeded BERT-style init, N(0, 0.02)), inputs, the oracle's outputs and its per-cross-layer median
    softmax row maximum."""
    key = (kv, gain)
    if key in _CASES:
        return _CASES[key]
    ocfg = O.QFormerCfg(enc_width=1408)
    w = O.init_weights(ocfg, seed=3, perturb=False) if gain is None else _peaked_weights(ocfg, seed=3, gain=gain)
    n, L = 3, 8
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(n, kv, 1408, generator=g)
    ids = torch.randint(1000, 30000, (n, L), generator=g)
    att = torch.ones(n, 32 + L, dtype=torch.long)
    enc = _qformer(dev, w).modality_ln(feats.to(dev))
    enc_ref = enc.float().cpu()           # the exact operand the kernels read
    collect = {}
    h = O.qformer_forward(w, ocfg, ids, att, w["query_tokens"].expand(n, -1, -1), enc_ref, collect=collect)
    _, logit_ref = O.cosine_scores(h[:, :32], h[:, 32])
    medians = [_cross_probabilities(w, ocfg, collect, enc_ref, i).max(dim=-1).values.median().item() for i in ocfg.cross_layers()]
    _CASES[key] = dict(w=w, ids=ids.to(dev), att=att.to(dev), enc=enc, logit_ref=logit_ref, medians=medians)
    return _CASES[key]


def _run(qf, c):
    res = qf.forward_fused(c["ids"], c["att"], c["enc"], want_query=True, want_cls=True)
    torch.cuda.synchronize()
    assert torch.isfinite(res["query"]).all()
    return res


def _dlogit(res, c):
    _, logit = O.cosine_scores(res["query"].cpu(), res["cls"].cpu())
    return (logit - c["logit_ref"]).abs().max().item() / c["logit_ref"].abs().max().item()


@pytest.mark.parametrize("kv", [2100, 300])
@pytest.mark.parametrize("gain", [1.0, 4.0, 7.0])
def test_probe_medians_match_the_oracle(dev, kv, gain):
    c = _case(dev, kv, gain)
    qf = _qformer(dev, c["w"], "auto")
    assert qf.cross_precision_report()["resolved"] is None and qf.cross_precision_report()["probes"] == 0
    _run(qf, c)
    rep = qf.cross_precision_report()
    print("probe", kv, gain, rep, "oracle", [round(m, 4) for m in c["medians"]])
    assert rep["mode"] == "auto" and rep["probes"] == 1 and len(rep["median_pmax"]) == len(c["medians"]) == 6
    for got, want in zip(rep["median_pmax"], c["medians"]):
        assert abs(got - want) <= MEDIAN_TOL, (got, want)
    assert rep["resolved"] == ("split" if max(rep["median_pmax"]) >= 0.5 else "op")


@pytest.mark.parametrize("kv", [2100, 300])
def test_diffuse_weights_resolve_to_op_bit_identically(dev, kv):
    c = _case(dev, kv, None)
    ref = _run(_qformer(dev, c["w"], "op"), c)
    qf = _qformer(dev, c["w"], "auto")
    first = _run(qf, c)
    assert qf.cross_precision_report()["resolved"] == "op"
    second = _run(qf, c)
    for res in (first, second):
        assert torch.equal(res["query"], ref["query"]) and torch.equal(res["cls"], ref["cls"])
    rep = qf.cross_precision_report()
    assert rep["probes"] == 1 and rep["resolved"] == "op" and max(rep["median_pmax"]) < 0.5


@pytest.mark.parametrize("kv,gain", PEAKED_CASES)
def test_peaked_weights_meet_the_logit_bar(dev, kv, gain):
    c = _case(dev, kv, gain)
    qf = _qformer(dev, c["w"], "auto")
    first = _run(qf, c)
    second = _run(qf, c)
    rep = qf.cross_precision_report()
    d1, d2 = _dlogit(first, c), _dlogit(second, c)
    print("auto", kv, gain, rep["resolved"], f"dlogit {d1:.2e} {d2:.2e}", [round(m, 3) for m in rep["median_pmax"]])
    assert d1 <= LOGIT_RTOL and d2 <= LOGIT_RTOL, (d1, d2)
    assert rep["probes"] == 1
    if gain >= 5:
        assert rep["resolved"] == "split"
    # the probing call already returns the resolved precision's outputs
    assert torch.equal(first["query"], second["query"]) and torch.equal(first["cls"], second["cls"])


def test_weight_upload_reprobes(dev):
    diffuse, peaked = _case(dev, 300, None), _case(dev, 300, 5.0)
    split_ref = _run(_qformer(dev, peaked["w"], "split"), peaked)
    qf = _qformer(dev, diffuse["w"], "auto")
    _run(qf, diffuse)
    assert qf.cross_precision_report()["resolved"] == "op"
    _load(qf, peaked["w"])
    qf.sync_weights()
    assert qf.cross_precision_report()["resolved"] is None      # stale until the next forward
    res = _run(qf, peaked)
    assert qf.cross_precision_report()["resolved"] == "split"
    assert torch.equal(res["query"], split_ref["query"]) and torch.equal(res["cls"], split_ref["cls"])
    assert _dlogit(res, peaked) <= LOGIT_RTOL
    _load(qf, diffuse["w"])
    _run(qf, diffuse)
    rep = qf.cross_precision_report()
    assert rep["resolved"] == "op" and rep["probes"] == 3
    _run(qf, diffuse)
    assert qf.cross_precision_report()["probes"] == 3


def test_threshold_option(dev):
    c = _case(dev, 300, 4.0)                 # median row maximum ~0.6
    qf = _qformer(dev, c["w"], "auto")
    from mraudio_amd._lib import MraError

    with pytest.raises(MraError):
        qf.set_option("auto_split_pmax_milli", 1001)
    qf.set_option("auto_split_pmax_milli", 1000)
    _run(qf, c)
    assert qf.cross_precision_report()["resolved"] == "op"
    qf.set_option("auto_split_pmax_milli", 500)
    qf.set_cross_precision("auto")           # forces a new probe
    assert qf.cross_precision_report()["resolved"] is None
    _run(qf, c)
    rep = qf.cross_precision_report()
    assert rep["resolved"] == "split" and rep["probes"] == 2


def test_kv_cache_mode_and_short_kv(dev):
    diffuse, peaked = _case(dev, 300, None), _case(dev, 300, 5.0)
    ref = _run(_qformer(dev, diffuse["w"], "op", "kv_cache"), diffuse)
    qf = _qformer(dev, diffuse["w"], "auto", "kv_cache")
    first, second = _run(qf, diffuse), _run(qf, diffuse)
    assert qf.cross_precision_report()["resolved"] == "op"
    for res in (first, second):   # the probe ran the folded form; the call still returns the K/V-cache form's bits
        assert torch.equal(res["query"], ref["query"]) and torch.equal(res["cls"], ref["cls"])
    split_ref = _run(_qformer(dev, peaked["w"], "split", "kv_cache"), peaked)
    qf = _qformer(dev, peaked["w"], "auto", "kv_cache")
    res = _run(qf, peaked)
    assert qf.cross_precision_report()["resolved"] == "split" and _dlogit(res, peaked) <= LOGIT_RTOL
    assert torch.equal(res["query"], split_ref["query"]) and torch.equal(res["cls"], split_ref["cls"])


def _pair_rc(qa, qb, c):
    """mra_qformer_forward_pair's return code (it refuses the handles before it looks at the workspace)."""
    from mraudio_amd._lib import current_stream, lib, ptr

    enc, ids, att = c["enc"], c["ids"], c["att"]
    n, kv = int(enc.shape[0]), int(enc.shape[1])
    outs = [torch.empty(n, 32, 768, device=enc.device) for _ in range(2)]
    cls = [torch.empty(n, 768, device=enc.device) for _ in range(2)]
    return int(lib().mra_qformer_forward_pair(qa._handle, qb._handle, ptr(ids), ptr(att), ptr(enc), ptr(enc), n, int(ids.shape[1]), kv, kv,
                                              ptr(outs[0]), ptr(cls[0]), ptr(outs[1]), ptr(cls[1]), None, C.c_size_t(0), current_stream()))


def test_pair_forward_refuses_unresolved_and_split(dev):
    diffuse, peaked = _case(dev, 300, None), _case(dev, 300, 5.0)
    op = _qformer(dev, diffuse["w"], "op")
    pending = _qformer(dev, diffuse["w"], "auto")
    assert _pair_rc(pending, op, diffuse) == MRA_ESTATE
    split = _qformer(dev, peaked["w"], "auto")
    _run(split, peaked)
    assert split.cross_precision_report()["resolved"] == "split"
    assert _pair_rc(split, op, diffuse) == MRA_ESTATE
    assert _pair_rc(op, split, diffuse) == MRA_ESTATE


def _smoke_inputs():
    bs, num = 1, 4
    g = torch.Generator().manual_seed(7)
    feats = {"video": torch.randn(bs, num, 257, 1408, generator=g), "audio": torch.randn(bs, num, 256, 768, generator=g)}
    samples = {"video_embeds": feats["video"], "audio_embeds": feats["audio"],
               "text_input": ["Query: a person opens the door.\nGiven the video and the query, find the relevant windows.\nRelevant windows: "],
               "timestamps": [[0, 2, 5, 7]], "duration": [10]}
    return bs, num, feats, samples


def _check_smoke(model, out, bs, num, feats, samples):
    """smoke()'s bars: |dz| < 2e-2, |dlogit| < 2e-3, fused < 2e-3, spans equal."""
    from mraudio_amd.models.xinstructblip import ENC_WIDTH

    text = model.tokenizer(samples["text_input"], padding="longest", truncation=True, max_length=128, return_tensors="pt")
    ids, tm = text.input_ids.repeat(num, 1), text.attention_mask.repeat(num, 1)
    cfgs = {m: O.QFormerCfg(enc_width=ENC_WIDTH[m]) for m in ("video", "audio")}
    ws = {"video": O.init_weights(cfgs["video"], seed=0, perturb=True), "audio": O.init_weights(cfgs["audio"], seed=1, perturb=True)}
    ref = O.encode_fuse_score(ws, cfgs, {m: feats[m].reshape(bs * num, *feats[m].shape[2:]) for m in ("audio", "video")}, ids, tm, bs, num)
    for m in ("video", "audio"):
        assert (out["z"][m].cpu() - ref["z"][m]).abs().max().item() < 2e-2
        assert (out["logit"][m].cpu() - ref["logit"][m]).abs().max().item() < 2e-3
    assert (out["fused"].cpu() - ref["fused"]).abs().max().item() < 2e-3
    assert [tuple(s) for s in out["spans"].cpu().tolist()] == [tuple(s) for s in ref["spans"]]


def test_model_auto_precision_at_smoke_shape(dev):
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    bs, num, feats, samples = _smoke_inputs()
    model = XInstructBLIP(seed=0, perturb=True, device=dev, cross_precision="auto")
    out = model.encode_fuse(samples)
    torch.cuda.synchronize()
    rep = model.cross_precision_report()
    print("model auto", rep)
    assert all(r["mode"] == "auto" and r["probes"] == 1 and r["resolved"] in ("op", "split") for r in rep.values())
    _check_smoke(model, out, bs, num, feats, samples)


def test_model_pair_forward_under_auto(dev):
    from mraudio_amd.models.xinstructblip import XInstructBLIP

    bs, num, feats, samples = _smoke_inputs()
    model = XInstructBLIP(seed=0, perturb=True, device=dev, cross_precision="auto")
    model.pair_forward = True
    for _ in range(2):   # unresolved: the two-forward route (it probes); then the pair route where both resolved to op
        out = model.encode_fuse(samples)
        torch.cuda.synchronize()
        _check_smoke(model, out, bs, num, feats, samples)
    assert all(r["probes"] == 1 for r in model.cross_precision_report().values())
