"""CPU suite: host-side logic that needs no GPU (sharding, tokenizer, processors' integer outputs,
span parsing pinned to the reference's own functions through tests/golden/integer_kats.json)."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from mraudio_amd import parallel
from mraudio_amd.models.xinstructblip import HashTokenizer
from mraudio_amd.processors.alpro_processors import AlproVideoEvalProcessor_Stamps, frame_indices, timestamps_from_indices
from mraudio_amd.qformer import QFormerConfig, draw_seeded, seeded_parameter_order
from mraudio_amd.utils import spans
from oracle import qformer_ref as O


def test_seeded_recipe_is_the_oracles():
    """The product's synthetic init must draw the same tensors as the checker's recipe."""
    cfg, ocfg = QFormerConfig(enc_width=768), O.QFormerCfg(enc_width=768)
    mine = seeded_parameter_order(cfg)
    theirs = [(n, k) for n, _, k in O.weight_names(ocfg)]
    assert mine == theirs
    small = O.QFormerCfg(enc_width=64, layers=2, vocab=50, max_pos=16, hidden=256, heads=4, inter=512, llm_hidden=256)
    w = O.init_weights(small, seed=5, perturb=True)
    g = torch.Generator().manual_seed(5)
    for name, shape, kind in O.weight_names(small):
        assert torch.equal(draw_seeded(g, shape, kind, True), w[name]), name
    assert torch.equal(draw_seeded(g, (1, 32, 256), "w", True), w["query_tokens"])
    assert torch.equal(draw_seeded(g, (64,), "g", True), w["ln.weight"])
    assert torch.equal(draw_seeded(g, (64,), "z", True), w["ln.bias"])
    assert torch.equal(draw_seeded(g, (256, 256), "w", True), w["llm_proj.weight"])
    assert torch.equal(draw_seeded(g, (256,), "b", True), w["llm_proj.bias"])


def test_shard_ranges_cover_in_order():
    for n in (0, 1, 7, 32, 33, 256):
        for ws in (1, 2, 3, 8):
            blocks = [parallel.shard_range(n, r, ws) for r in range(ws)]
            assert blocks[0][0] == 0 and blocks[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
            sizes = [hi - lo for lo, hi in blocks]
            assert max(sizes) - min(sizes) <= 1 and sizes == parallel.shard_sizes(n, ws)
    assert parallel.shard_range(256, 3, 8) == (96, 128)


def test_hash_tokenizer_contract():
    tok = HashTokenizer(truncation_side="left")
    out = tok(["find the door", "a much longer query about a person opening the red door slowly"], padding="longest",
              truncation=True, max_length=8, return_tensors="pt")
    assert out.input_ids.shape == out.attention_mask.shape == (2, 8)
    assert out.input_ids[0, 0] == 101 and out.input_ids[1, 0] == 101 and out.input_ids[1, -1] == 102
    assert out.attention_mask[0].tolist() == [1, 1, 1, 1, 1, 0, 0, 0]
    assert (out.input_ids[0, 5:] == 0).all()
    assert tok(["Door"]).input_ids.tolist() == tok(["door"]).input_ids.tolist()  # uncased
    assert int(out.input_ids.max()) < 30523 and len(tok) == 30523
    # left truncation keeps the tail of the prompt (reference init_tokenizer(truncation_side="left"))
    long = tok(["one two three four five six seven eight nine ten"], max_length=6)
    assert long.input_ids[0, 1:5].tolist() == tok(["seven eight nine ten"]).input_ids[0, 1:5].tolist()


def test_frame_indices_and_timestamps_known_answers():
    # processors/alpro_processors.py:25  np.linspace(0, vlen, n, endpoint=False).astype(int)
    assert frame_indices(100, 8).tolist() == [0, 12, 25, 37, 50, 62, 75, 87]
    assert frame_indices(5, 60).tolist() == [0, 1, 2, 3, 4]            # n_frms clipped to vlen
    assert frame_indices(1800, 60)[:4].tolist() == [0, 30, 60, 90]
    # utils/mr_dataset.py:44  round(idx / fps): Python rounds half to even
    assert timestamps_from_indices([0, 12, 25, 37, 50, 62, 75, 87], 25.0) == [0, 0, 1, 1, 2, 2, 3, 3]
    assert timestamps_from_indices([15, 45], 30.0) == [0, 2]
    import random
    r = frame_indices(100, 4, "random", random.Random(0))
    assert len(r) == 4 and all(25 * i <= v < 25 * (i + 1) for i, v in enumerate(r))
    with pytest.raises(NotImplementedError):
        frame_indices(10, 2, "other")


def test_eval_processor_pads_with_last_frame():
    def reader(path, h, w):
        frames = np.arange(3, dtype=np.float32).reshape(3, 1, 1, 1) * np.ones((3, h, w, 3), dtype=np.float32)
        return frames, 2.0

    proc = AlproVideoEvalProcessor_Stamps(image_size=4, n_frms=5, reader=reader)
    clip, idx, fps = proc("x.mp4")
    assert clip.shape == (3, 5, 4, 4) and list(idx) == [0, 1, 2] and fps == 2.0
    assert torch.equal(clip[:, 3], clip[:, 2]) and torch.equal(clip[:, 4], clip[:, 2])


def test_span_parsing_matches_reference_kats(golden_dir):
    kat = json.load(open(os.path.join(golden_dir, "integer_kats.json")))
    for row in kat["post_process"]:
        p = spans.post_process(row["in"])
        assert p == row["post"], row
        assert spans.moment_str_to_list(p) == row["list"], row
    for row in kat["convert_percentages"]:
        assert spans.convert_percentages_to_second(row["in"], row["duration"]) == row["out"]
    for row in kat["iou_cross"]:
        np.testing.assert_allclose(spans.temporal_iou_cross(np.array(row["a"]), np.array(row["b"])), np.array(row["iou"]))
    for row in kat["iou_paired"]:
        np.testing.assert_allclose(spans.temporal_iou_paired(np.array(row["a"]), np.array(row["b"])), np.array(row["iou"]))


def test_generated_strings_round_trip_through_the_parser():
    s = O.spans_to_text([(1, 3), (0, 0)], [[0, 2, 5, 7], [4, 6, 8, 9]])
    assert s == ["[[2, 7]]", "[[4, 4]]"]
    assert [spans.moment_str_to_list(spans.post_process(x)) for x in s] == [[[2, 7]], [[4, 4]]]


def test_eva_vit_g_geometry_cpu():
    """Row A1 callee: stock-PyTorch EVA ViT-g restated with the geometry LAVIS instantiates
    (reference models/xinstructblip.py:658-666): 257 tokens x 1408, 39 blocks, 520.7 GF / frame."""
    from mraudio_amd.models.eva_vit import EvaViTg, create_eva_vit_g

    m = EvaViTg(depth=2).eval()
    with torch.no_grad():
        y = m(torch.randn(2, 3, 224, 224))
    assert y.shape == (2, 257, 1408) and m.num_features == 1408
    assert abs(EvaViTg.flops_per_frame(type("S", (), {"pos_embed": torch.zeros(1, 257, 1408), "num_features": 1408,
                                                        "blocks": [type("B", (), {"fc1": type("F", (), {"out_features": 6144})()})()] * 39})()) / 1e9 - 520.7) < 0.1
    import inspect
    assert list(inspect.signature(create_eva_vit_g).parameters)[:4] == ["img_size", "drop_path_rate", "use_checkpoint", "precision"]


def test_text_output_windows_float_and_multi_window():
    """the reference's preprocessing writes float windows (``save_float=True``) and QVHighlights rows
    hold several windows; the training target is the union of all of them."""
    from mraudio_amd.models.xinstructblip import XInstructBLIP as X

    assert X.parse_windows("[[24.3, 30.4]]") == [[24.3, 30.4]]
    assert X.parse_windows("[[0, 10], [20, 30]]") == [[0.0, 10.0], [20.0, 30.0]]
    assert X.parse_windows("[[12, 5]]") == [[5.0, 12.0]]            # reversed bounds are swapped, as utils/utils.py does
    assert X.parse_windows("[[-1, -1]]") == []                       # "no window"
    with pytest.raises(ValueError):
        X.parse_windows("no windows here")
    stub = type("S", (), {"_device": torch.device("cpu"), "parse_windows": X.parse_windows})()
    samples = {"timestamps": [[0, 5, 10, 15, 20, 25, 30]], "text_output": ["[[4.5, 10.2], [24.9, 30]]"]}
    tgt = X._targets(stub, samples, 1, 7)
    assert tgt.tolist() == [[0.0, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0]]


def test_prompt_rows_in_the_three_orders_against_explicit_loops():
    """The chain's text rows: ``compat_repeat`` (row k carries prompt k % bs), aligned (k // num) and multi-query (row (b * T + t) * P + p
    carries prompt p of video b), the attention mask with the query-token ones in front of each row's own text mask."""
    from mraudio_amd.models.xinstructblip import _prompt_rows

    bs, num, P, L, Q = 2, 3, 2, 4, 32
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1000, 30000, (bs, L), generator=g)
    tmask = torch.tensor([[1, 1, 1, 0], [1, 1, 0, 0]])

    def check(got, want_ids, want_tm):
        got_ids, att = got
        assert got_ids.tolist() == want_ids and att.dtype == torch.long and att.shape == (len(want_ids), Q + L)
        assert att.tolist() == [[1] * Q + row for row in want_tm]

    n = bs * num
    check(_prompt_rows(ids, tmask, Q, num, tile=True), [ids[k % bs].tolist() for k in range(n)], [tmask[k % bs].tolist() for k in range(n)])
    check(_prompt_rows(ids, tmask, Q, num), [ids[k // num].tolist() for k in range(n)], [tmask[k // num].tolist() for k in range(n)])
    assert _prompt_rows(ids, tmask, Q, num, tile=True)[0][1].tolist() == ids[1].tolist() != ids[0].tolist() == _prompt_rows(ids, tmask, Q, num)[0][1].tolist()
    ids_p = torch.randint(1000, 30000, (bs * P, L), generator=g)                     # row b * P + p
    tm_p = torch.tensor([[1, 1, 1, 1], [1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0]])
    order = [b * P + p for b in range(bs) for t in range(num) for p in range(P)]
    check(_prompt_rows(ids_p, tm_p, Q, num, P), [ids_p[r].tolist() for r in order], [tm_p[r].tolist() for r in order])
    check(_prompt_rows(ids, tmask, Q), ids.tolist(), tmask.tolist())                # no position count: the rows as given


def test_timestamps_default_and_tensor_valued():
    from mraudio_amd.models.xinstructblip import _timestamps

    assert _timestamps({}, 2, 3) == [[0, 1, 2], [0, 1, 2]]
    assert _timestamps({"timestamps": None}, 1, 2) == [[0, 1]]
    assert _timestamps({"timestamps": [torch.tensor([0, 2, 4]), (1, 3, 5)]}, 2, 3) == [[0, 2, 4], [1, 3, 5]]
    assert _timestamps({"timestamps": torch.tensor([[0.5, 2.5], [1.0, 3.0]])}, 2, 2) == [[0.5, 2.5], [1.0, 3.0]]


def test_single_query_targets_are_row_0_of_the_multi_query_targets():
    from mraudio_amd.models.xinstructblip import XInstructBLIP as X

    stub = type("S", (), {"_device": torch.device("cpu"), "parse_windows": X.parse_windows})()
    stamps = [[0, 5, 10, 15, 20, 25, 30], torch.tensor([0.0, 2.5, 5.0, 7.5, 10.0, 12.5, 15.0])]
    texts = ["[[4.5, 10.2], [24.9, 30]]", "[[-1, -1]]", "[[2.5, 7.5]]", "[[12, 5]]"]
    for ts in stamps:
        want = [[float(any(min(a, b) <= float(t) <= max(a, b) for a, b in X.parse_windows(txt))) for t in ts] for txt in texts]
        multi = X._multi_targets(stub, {"timestamps": [ts]}, [texts], 7)
        assert len(multi) == 1 and multi[0].tolist() == want and any(map(any, want))
        for p, txt in enumerate(texts):
            single = X._targets(stub, {"timestamps": [ts], "text_output": [txt]}, 1, 7)
            assert torch.equal(single[0], X._multi_targets(stub, {"timestamps": [ts]}, [[txt] + texts], 7)[0][0]) and single.tolist() == [want[p]]
    # no timestamps: positions 0 .. num - 1; no text_output: no window
    assert X._targets(stub, {"text_output": ["[[1, 2]]", "[[0, 0]]"]}, 2, 4).tolist() == [[0.0, 1.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0]]
    assert X._targets(stub, {}, 2, 3).tolist() == [[0.0] * 3] * 2


def test_batched_encode_is_sample_major_and_sharded():
    """Row A1: the reference's T sequential encoder calls at batch B (models/xinstructblip.py:262-275) followed by
    ``cat(embeds)[indices]`` (:281-285) equal ONE sample-major [B*T] batch; a rank's [lo, hi) block touches only
    its own frames."""
    from mraudio_amd.models.xinstructblip import XInstructBLIP as X

    calls = []

    def enc(x):                       # stand-in encoder: per-frame mean -> [n, 2, 3]
        calls.append(int(x.shape[0]))
        return x.flatten(1).mean(1)[:, None, None].expand(-1, 2, 3).clone()

    B, T = 2, 5
    video = torch.arange(B * 3 * T * 4 * 4, dtype=torch.float32).view(B, 3, T, 4, 4)
    stub = type("S", (), {"_device": torch.device("cpu"), "encode_chunk": 4, "video_encoder": staticmethod(enc), "audio_encoder": staticmethod(enc)})()
    raw, idx, bs, num = X._encode(stub, {"video": video}, "video")
    assert idx is None and (bs, num) == (B, T) and raw.shape == (B * T, 2, 3) and calls == [4, 4, 2]
    # the reference's order: per-position loop, cat, then the sample-major gather
    frames = torch.cat([enc(video[:, :, j]) for j in range(T)])
    ref = frames[torch.tensor(O.reorder_indices(B, T))]
    assert torch.equal(raw, ref)
    calls.clear()
    part, _, _, _ = X._encode(stub, {"video": video}, "video", 3, 8)
    assert torch.equal(part, ref[3:8]) and sum(calls) == 5          # only this rank's five frames were encoded
    audio = torch.randn(B, T, 6, 128)
    ra, _, bs, num = X._encode(stub, {"audio": audio}, "audio")
    fa = torch.cat([enc(audio[:, j]) for j in range(T)])[torch.tensor(O.reorder_indices(B, T))]
    assert torch.equal(ra, fa) and (bs, num) == (B, T)
    pre = torch.randn(B, T, 7, 16)
    rp, _, _, _ = X._encode(stub, {"video_embeds": pre}, "video", 2, 9)
    assert torch.equal(rp, pre.reshape(B * T, 7, 16)[2:9])


def test_gemm_plan_matrix_needs_no_gpu():
    """`kernel_check plan` walks gemm_plan (tile, kernel family, grid and every refusal of launch_gemm) over its fixed matrix of
    problems before any HIP call; it checks what holds for every accepted launch and how many the matrix accepts."""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "kernel_check")
    assert os.path.exists(exe), f"{exe} is missing: build() makes it"
    r = subprocess.run([exe, "plan"], capture_output=True, text=True, timeout=300)
    last = r.stdout.strip().splitlines()[-1]
    assert r.returncode == 0 and last.startswith("plan: ") and last.endswith(" 0 failed"), (r.returncode, last, r.stderr[-500:])
