"""No GPU: what the multi-prompt path rests on before a kernel runs -- the bound of ``tests/multi_query_cases.py`` against an emulation of
the core's arithmetic, the mutants that bound catches, the grouping of annotation lines by video, the (b, t, p) -> (b, p, t) order of the
scored rows, and the argument checks of the new ABI entries that need no device."""
import ctypes as C

import pytest
import torch

import multi_query_cases as M
from mraudio_amd import _lib
from mraudio_amd.utils import mr_dataset as D

KVS = (1, 33, 257)
ENC_ITEMS, P, HEADS = 2, 3, 2


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("kv", KVS)
def test_emulated_core_sits_inside_half_of_the_bound(kv, dtype):
    for kind in M.families_for(kv):
        q, k, v = M.make_multi(kind, ENC_ITEMS, P, HEADS, kv, dtype)
        ref, bound = M.multi_ref(q, k, v, P)
        r = M.worst_ratio(M.emulate(q, k, v, P), ref, bound)
        print(f"{kind} kv={kv} {dtype}: emulation / bound = {r:.3f}")
        assert r <= 0.5, (kind, kv, dtype, r)   # above half: the bound does not fit this kernel -- do not widen it


def test_inputs_differ_per_encoder_item_and_per_prompt_slot():
    for kind in M.families_for(257):
        q, k, v = M.make_multi(kind, ENC_ITEMS, P, HEADS, 257)
        assert not torch.equal(k[0], k[1]) and not torch.equal(v[0], v[1]), kind
        for i in range(ENC_ITEMS):
            for a in range(P):
                for b in range(a + 1, P):
                    assert not torch.equal(q[i * P + a], q[i * P + b]), (kind, i, a, b)


def _mutant_ratio(mutant, kind, kv, dtype=torch.float16):
    q, k, v = M.make_multi(kind, ENC_ITEMS, P, HEADS, kv, dtype)
    ref, bound = M.multi_ref(q, k, v, P)
    return M.worst_ratio(M.emulate(q, k, v, P, mutant=mutant), ref, bound)


@pytest.mark.parametrize("kv", KVS)
def test_mutant_kv_of_the_next_item_breaks_mild(kv):
    assert _mutant_ratio("kv_next", "mild", kv) > 1.0


@pytest.mark.parametrize("kv", (33, 257))
def test_mutant_q_of_the_next_prompt_slot_breaks_mild(kv):
    # (kv = 1 cannot see it: one key, the output is v whatever the query)
    assert _mutant_ratio("q_next", "mild", kv) > 1.0
    assert _mutant_ratio("q_next", "peaked", kv) > 1.0


@pytest.mark.parametrize("kv", (33, 257))
def test_mutant_unmasked_tail_breaks_constant(kv):
    # the padding rows of the last tile repeat the last key: uniform rows then overweight v[kv - 1]
    # (kv = 1 cannot see it: every padding row is the only key)
    assert _mutant_ratio("tail", "constant", kv) > 1.0
    assert _mutant_ratio("tail", "mild", kv) > 1.0


# ---- grouping by video ------------------------------------------------------------------------------------------------------------
ANN = [{"vid": v, "qid": i, "query": f"q{i}", "relevant_windows": [[i, i + 1]]} for i, v in enumerate("abacbbadab")]


def test_group_by_video_order_of_first_appearance_and_chunking():
    assert D.group_by_video(ANN, 16) == [[0, 2, 6, 8], [1, 4, 5, 9], [3], [7]]
    assert D.group_by_video(ANN, 3) == [[0, 2, 6], [8], [1, 4, 5], [9], [3], [7]]
    assert D.group_by_video(ANN, 1) == [[0], [2], [6], [8], [1], [4], [5], [9], [3], [7]]
    assert D.group_by_video([], 4) == []
    with pytest.raises(ValueError):
        D.group_by_video(ANN, 0)


def test_restore_order_inverts_the_grouping():
    for mq in (1, 2, 3, 16):
        groups = D.group_by_video(ANN, mq)
        results = [[f"r{i}" for i in g] for g in groups]
        assert D.restore_order(groups, results) == [f"r{i}" for i in range(len(ANN))]
    with pytest.raises(ValueError):
        D.restore_order([[0, 1]], [["x"]])


def test_ragged_padding_and_dropping():
    padded, counts = D.pad_queries([["a", "b", "c"], ["d"], ["e", "f"]])
    assert padded == [["a", "b", "c"], ["d", "d", "d"], ["e", "f", "f"]] and counts == [3, 1, 2]
    assert D.drop_padding(padded, counts) == [["a", "b", "c"], ["d"], ["e", "f"]]
    with pytest.raises(ValueError):
        D.pad_queries([["a"], []])


class _Base(torch.utils.data.Dataset):
    def __init__(self):
        self.annotation = ANN
        self.loads = []

    def __len__(self):
        return len(ANN)

    def __getitem__(self, i):
        self.loads.append(i)
        a = ANN[i]
        return {"text_input": D.build_prompt(a["query"]), "text_output": str(a["relevant_windows"]), "qid": a["qid"], "query": a["query"],
                "vid": a["vid"], "duration": 10, "timestamps": [0, 1], "video_embeds": torch.full((2, 1, 4), float(ord(a["vid"])))}


def test_video_grouped_dataset_loads_each_video_once_per_group():
    base = _Base()
    ds = D.VideoGroupedDataset(base, max_queries=3)
    assert len(ds) == 6
    recs = [ds[g] for g in range(len(ds))]
    assert base.loads == [0, 8, 1, 9, 3, 7]                    # one load per group: the group's first line
    assert recs[0]["qid"] == [0, 2, 6] and recs[0]["index"] == [0, 2, 6] and recs[0]["vid"] == "a"
    assert recs[0]["text_input"] == [D.build_prompt(f"q{i}") for i in (0, 2, 6)]
    assert recs[2]["text_output"] == [str([[i, i + 1]]) for i in (1, 4, 5)]
    batch = D.collate_grouped(recs[:2])
    assert batch["video_embeds"].shape == (2, 2, 1, 4) and batch["query"] == [["q0", "q2", "q6"], ["q8"]] and batch["vid"] == ["a", "a"]


def test_synthetic_annotation_matches_its_records():
    ds = D.SyntheticMRDataset(3, T=6, modalities=("audio",), kv_audio=2)
    for i, a in enumerate(ds.annotation):
        rec = ds[i]
        assert (a["qid"], a["query"], a["vid"], str(a["relevant_windows"])) == (rec["qid"], rec["query"], rec["vid"], rec["text_output"])


def test_bpt_index_against_a_brute_force_loop():
    for bs, num, p in ((1, 1, 1), (2, 4, 3), (3, 5, 2), (2, 1, 4)):
        idx = D.bpt_index(bs, num, p).tolist()
        want = [(b * num + t) * p + s for b in range(bs) for s in range(p) for t in range(num)]
        assert idx == want
        rows = torch.arange(bs * num * p) * 10
        out = rows[D.bpt_index(bs, num, p)]
        for b in range(bs):
            for s in range(p):
                for t in range(num):
                    assert out[(b * p + s) * num + t].item() == ((b * num + t) * p + s) * 10


# ---- the ABI entries without a device ---------------------------------------------------------------------------------------------
def test_multi_entries_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.mra_qformer_multi_workspace_bytes(None, 2, 3, 9, 257) == 0
    assert L.mra_qformer_forward_multi(None, None, None, None, 2, 3, 9, 257, None, None, None, 0, None) == -1
    assert b"null handle" in L.mra_last_error()
    # prompts = 0 is refused on its own ground, ahead of everything else (no handle exists without a device)
    assert L.mra_qformer_forward_multi(None, None, None, None, 2, 0, 9, 257, None, None, None, 0, None) == -1
    assert b"prompts" in L.mra_last_error()
    # the core's debug entry: host buffers stand in for device memory, every call below must return before it would launch
    fake = C.create_string_buffer(1 << 16)
    assert L.mra_debug_shared_kv_attention(fake, fake, fake, _lib.MRA_F16, 1, 0, 1, 8, 0, fake, None, 0, None) == -1
    assert b"prompts" in L.mra_last_error()
    assert L.mra_debug_shared_kv_attention(fake, fake, fake, _lib.MRA_F16, 1, 1, 1, 8, 2, fake, None, 0, None) == -1
    assert L.mra_debug_shared_kv_attention(fake, fake, fake, _lib.MRA_F32, 1, 1, 1, 8, 0, fake, None, 0, None) == -1
    assert L.mra_debug_shared_kv_attention(None, None, None, _lib.MRA_F16, 0, 1, 1, 8, 0, None, None, 0, None) == 0   # no items: no-op
    assert L.mra_debug_shared_kv_workspace_bytes(2, 4, 12, 257, 0) == 0 and L.mra_debug_shared_kv_workspace_bytes(2, 4, 12, 257, 1) == 0
    assert L.mra_debug_shared_kv_workspace_bytes(1, 5, 1, 2049, 0) > 0 and L.mra_debug_shared_kv_workspace_bytes(1, 5, 1, 2049, 1) > 0
    assert L.mra_debug_shared_kv_workspace_bytes(1, 0, 1, 2049, 1) == 0
