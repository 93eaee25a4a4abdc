"""The one-token attention without a GPU (``-m "not gpu"``): the fp32 emulation of csrc/decode_attn.hip sits inside the derived bounds of
tests/decode_attn_cases.py and every named mutant lands outside; the table covers what it says; the torch route of
``mraudio_amd/models/lm_decode.py`` is the float64 definition; both entries refuse bad arguments with host pointers before any launch; the
workspace formula is the header's."""
import ctypes as C
import itertools
import math

import pytest
import torch

import decode_attn_cases as DC
from mraudio_amd import _lib
from mraudio_amd.models import lm_decode as LD


def _id(dt):
    return str(dt).split(".")[-1]


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DC.DTYPES, ids=_id)
def test_emulation_sits_inside_every_bound(dtype):
    worst = [0.0, 0.0]
    for case in DC.cases():
        r = DC.ratios(*case, dtype, *DC.emulate(*case, dtype))
        assert max(r) <= 1.0, (case, r)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"{_id(dtype)}: worst |d| / bound of the emulation: out {worst[0]:.3f} lse {worst[1]:.3f}")
    assert all(w > 0.0 for w in worst)


@pytest.mark.parametrize("dtype", DC.DTYPES, ids=_id)
@pytest.mark.parametrize("mutant", DC.MUTANTS)
def test_mutants_land_outside_somewhere(mutant, dtype):
    worst = max(max(DC.ratios(*case, dtype, *DC.emulate(*case, dtype, mutant=mutant))) for case in DC.cases())
    assert worst > 1.0, (mutant, worst)


def test_table_covers_what_it_says():
    cs = DC.cases()
    assert len(cs) == len(DC.SEQS) * len(DC.MASKS) == len(set(cs))
    cols = {"B": [c[0] for c in cs], "heads": [(c[1], c[2]) for c in cs], "S": [c[3] for c in cs], "D": [c[4] for c in cs], "mask": [c[5] for c in cs]}
    values = {"B": DC.BATCHES, "heads": DC.HEADS, "S": DC.SEQS, "D": DC.DIMS, "mask": DC.MASKS}
    for a, b in itertools.combinations(cols, 2):                                    # every value of one meets every value of every other
        assert set(zip(cols[a], cols[b])) == set(itertools.product(values[a], values[b])), (a, b)
    assert DC.SEQS == (1, 63, 64, 65, 255, 256, 257, 515, 1041) and DC.chunks(256) == 1 and DC.chunks(257) == 2 and DC.chunks(1041) == 5
    seen = set()
    for case in cs:
        B, Hq, Hkv, S, D, mask = case
        c, ref = DC.make_case(*case, torch.bfloat16), DC.reference(*case, torch.bfloat16)
        lay = DC.layout(B, Hq, Hkv, S, D)
        assert lay["Smax"] > S and all(lay[n] % 8 == 0 and lay[n] >= D for n in ("k_ss", "v_ss", "q_sh", "o_sh")) and lay["q_sh"] > D < lay["o_sh"]
        att = torch.ones(B, S, dtype=torch.bool) if c["mask"] is None else c["mask"]
        dead = ~att[:, None, :, None].expand_as(c["k"])
        assert torch.isfinite(c["k"][~dead]).all() and torch.isfinite(c["v"][~dead]).all() and torch.isfinite(c["q"]).all()
        assert not torch.isfinite(c["k"][dead]).any() and not torch.isfinite(c["v"][dead]).any()
        assert torch.equal(ref["empty"], ~att.any(1)[:, None].expand(B, Hq))
        if mask == "row_masked":
            assert ref["empty"][B - 1].all() and (B == 1 or not ref["empty"][0].any())
            assert bool((ref["out"][B - 1] == 0).all()) and bool((ref["lse"][B - 1] == float("-inf")).all())
        if mask == "mid_chunk" and S > 2 * DC.C:
            assert not att[:, DC.C:2 * DC.C].any() and att[:, :DC.C].all() and att[:, 2 * DC.C:].all()
        if mask == "first_chunk" and S > DC.C:
            assert not att[:, :DC.C].any() and att[:, DC.C:].all()
        if mask == "last_only":
            assert att.sum(1).tolist() == [1] * B and att[:, -1].all()
        for b in range(B):
            for h in range(Hq):
                fam = c["family"][b][h]
                if ref["empty"][b, h]:
                    continue
                seen.add(fam)
                n = int(att[b].sum())
                if fam == "equal":                                                   # out = the mean of the attended V rows, lse = log count
                    assert abs(ref["lse"][b, h].item() - math.log(n)) < 1e-12
                    mean = c["v"][b, h // (Hq // Hkv)][att[b]].double().mean(0)
                    assert (ref["out"][b, h] - mean).abs().max() < 1e-12
                if fam in ("plus90", "minus90"):
                    assert abs(abs(ref["lse"][b, h].item()) - 90) < 12
    assert seen == set(DC.FAMILIES)


# ---- the torch route ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 8, 2, 65, 64, "holes"), (1, 4, 4, 257, 128, "null"), (3, 4, 2, 63, 64, "row_masked"), (3, 3, 3, 515, 128, "mid_chunk")])
@pytest.mark.parametrize("dtype", DC.DTYPES, ids=_id)
def test_torch_route_is_the_definition(case, dtype):
    B, Hq, Hkv, S, D, _ = case
    c, ref = DC.make_case(*case, dtype), DC.reference(*case, dtype)
    lay = DC.layout(B, Hq, Hkv, S, D)
    kbuf = torch.full((B, Hkv, lay["Smax"], lay["k_ss"]), float("nan"), dtype=dtype)           # the static-cache form: views of a longer buffer
    vbuf = torch.full((B, Hkv, lay["Smax"], lay["v_ss"]), float("inf"), dtype=dtype)
    kbuf[:, :, :S, :D], vbuf[:, :, :S, :D] = c["k"], c["v"]
    mask = None if c["mask"] is None else c["mask"][:, None, None, :]
    for hip in (False, None):                                                        # None on CPU tensors: the torch ops
        out = LD.decode_attention(c["q"][:, :, None, :], kbuf[:, :, :S, :D], vbuf[:, :, :S, :D], mask, c["scale"], hip=hip)
        assert out.shape == (B, Hq, 1, D) and out.dtype == dtype
        assert max(DC.ratios_against(ref, out[:, :, 0], None)) <= 1.0
    with pytest.raises(_lib.MraError, match="CUDA"):
        LD.decode_attention(c["q"][:, :, None, :], c["k"], c["v"], mask, c["scale"], hip=True)


def test_python_entry_refuses_malformed_calls():
    q, k = torch.zeros(2, 4, 1, 64), torch.zeros(2, 2, 9, 64)
    with pytest.raises(ValueError, match="expected"):
        LD.decode_attention(q[:, :, 0], k, k, None, 1.0)
    with pytest.raises(ValueError, match="expected"):
        LD.decode_attention(q, k, k[:, :, :8], None, 1.0)
    with pytest.raises(ValueError, match="mask"):
        LD.decode_attention(q, k, k, torch.ones(2, 1, 1, 8, dtype=torch.bool), 1.0)
    with pytest.raises(ValueError, match="mask"):
        LD.decode_attention(q, k, k, torch.zeros(2, 1, 1, 9), 1.0)                    # an additive float mask is not this entry's


# ---- the ABI entries without a device ---------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.lib()
    buf = C.create_string_buffer(1 << 16)
    p = (C.addressof(buf) + 15) // 16 * 16
    BF = _lib.MRA_BF16
    need = DC.workspace_bytes(2, 8, 300, 64)
    nan, inf = float("nan"), float("inf")

    def run(q=p, q_sb=512, q_sh=64, k=p, k_sb=4 * 300 * 64, k_sh=300 * 64, k_ss=64, v=p, v_sb=4 * 300 * 64, v_sh=300 * 64, v_ss=64, mask=p, mask_sb=300,
            B=2, Hq=8, Hkv=4, S=300, D=64, dt=BF, scale=0.125, out=p, o_sb=512, o_sh=64, lse=p, ws=p, nbytes=need):
        return lib.mra_decode_attention(q, q_sb, q_sh, k, k_sb, k_sh, k_ss, v, v_sb, v_sh, v_ss, mask, mask_sb, B, Hq, Hkv, S, D, dt, scale, out, o_sb,
                                        o_sh, lse, ws, nbytes, None)

    bad = [("null", dict(q=None)), ("null", dict(k=None)), ("null", dict(v=None)), ("null", dict(out=None)), ("null", dict(ws=None)),
           ("multiple of Hkv", dict(Hq=7)), ("multiple of Hkv", dict(Hkv=0)), ("1, 2, 4 or 8", dict(Hq=12)), ("1, 2, 4 or 8", dict(Hq=64)),
           ("D must", dict(D=32)), ("D must", dict(D=96)), ("D must", dict(D=256)), ("S must", dict(S=0)), ("negative B", dict(B=-1)),
           ("dtype", dict(dt=_lib.MRA_F32)), ("dtype", dict(dt=9)),
           ("16-byte aligned", dict(q=p + 8)), ("16-byte aligned", dict(k=p + 2)), ("16-byte aligned", dict(v=p + 4)), ("16-byte aligned", dict(out=p + 8)),
           ("16-byte aligned", dict(ws=p + 4)), ("4-byte aligned", dict(lse=p + 2)),
           ("strides", dict(q_sb=516)), ("strides", dict(q_sh=68)), ("strides", dict(k_sb=4)), ("strides", dict(k_sh=300 * 64 + 1)), ("strides", dict(k_ss=68)),
           ("strides", dict(v_sb=12)), ("strides", dict(v_sh=7)), ("strides", dict(v_ss=100)), ("strides", dict(o_sb=514)), ("strides", dict(o_sh=66)),
           ("< D", dict(k_ss=56)), ("< D", dict(v_ss=0)), ("< D", dict(k_ss=-64)),
           ("workspace too small", dict(nbytes=need - 1)), ("workspace too small", dict(nbytes=0)),
           ("scale", dict(scale=nan)), ("scale", dict(scale=inf)), ("scale", dict(scale=-inf))]
    for msg, kw in bad:
        assert run(**kw) == -1, kw
        assert msg.encode() in lib.mra_last_error(), (kw, lib.mra_last_error())
    # B == 0 launches nothing and needs nothing, not even pointers
    assert run(B=0, q=None, k=None, v=None, out=None, ws=None, nbytes=0) == 0


def test_workspace_bytes_agree_with_the_header_formula():
    lib = _lib.lib()
    shapes = [(c[0], c[1], c[3], c[4]) for c in DC.cases()] + [(2, 32, 5400, 128), (2, 32, 1900, 128), (0, 4, 9, 64), (64, 64, 100000, 128)]
    for B, Hq, S, D in shapes:
        assert lib.mra_decode_attention_workspace_bytes(B, Hq, S, D) == DC.workspace_bytes(B, Hq, S, D), (B, Hq, S, D)
    assert DC.workspace_bytes(2, 32, 5400, 128) * 30 < 2 * 2 * 32 * 5400 * 128 * 2        # a thirtieth of the K/V bytes one call reads
    for bad in ((-1, 4, 9, 64), (1, 0, 9, 64), (1, 4, 0, 64), (1, 4, 9, 32), (1, 4, 9, 96)):
        assert lib.mra_decode_attention_workspace_bytes(*bad) == 0
        assert b"decode_attention_workspace_bytes" in lib.mra_last_error()
