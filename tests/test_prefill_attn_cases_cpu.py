"""The prefill attention without a GPU (``-m "not gpu"``): the float64 definition of tests/prefill_attn_cases.py agrees with
``scaled_dot_product_attention`` under the explicit [Sq, Skv] bool mask; the fp32 emulation of csrc/prefill_attn.hip sits inside the derived
bounds and every named mutant lands outside; the table covers what it says; the torch route of ``mraudio_amd/models/lm_decode.py`` is the
definition; the entry refuses bad arguments with host pointers before any launch and writes nothing."""
import ctypes as C
import itertools
import math
import os
import re

import pytest
import torch

import prefill_attn_cases as PC
from mraudio_amd import _lib
from mraudio_amd.models import lm_decode as LD

SMALL = [c for c in PC.cases() if c[3] <= PC.QB + 1]           # the mutants are run where a case takes milliseconds


def _id(dt):
    return str(dt).split(".")[-1]


def test_constants_are_the_kernels():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mraudio_amd", "csrc", "kernels.h")).read()
    m = re.search(r"constexpr int PREFILL_QB = (\d+), PREFILL_KT = (\d+)", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (PC.QB, PC.KT)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in PC.cases() if c[3] in (2, PC.KT + 1, PC.QB + 1, 5, 3)], ids=str)
def test_float64_definition_against_sdpa_under_the_explicit_mask(case):
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    c, ref = PC.make_case(*case, torch.bfloat16), PC.reference(*case, torch.bfloat16)
    att = PC.attended(c["mask"], B, Sq, Skv, off)                                   # [B, Sq, Skv]
    G = Hq // Hkv
    some = att.any(1)[:, None, :, None]
    zero = torch.zeros((), dtype=torch.float64)
    kd = torch.where(some, c["k"].double(), zero).repeat_interleave(G, dim=1)
    vd = torch.where(some, c["v"].double(), zero).repeat_interleave(G, dim=1)
    want = torch.nn.functional.scaled_dot_product_attention(c["q"].double(), kd, vd, attn_mask=att[:, None], scale=c["scale"]).transpose(1, 2)
    live = ~ref["empty"].transpose(1, 2)                                            # [B, Sq, Hq]
    assert live.any() or case[7] == "row_masked"
    if live.any():
        assert (want[live] - ref["out"][live]).abs().max().item() <= 1e-12
    # the torch route in float64 is the same definition; rows without a key: +0 and -inf
    out, lse = LD.prefill_attention(c["q"].double(), c["k"].double(), c["v"].double(), None if c["mask"] is None else c["mask"][:, None, None, :],
                                    c["scale"], q_offset=off, want_lse=True)
    assert out.dtype == torch.float64
    if live.any():
        assert (out[live] - want[live]).abs().max().item() <= 1e-12
        assert (lse[~ref["empty"]] - ref["lse"][~ref["empty"]]).abs().max().item() <= 1e-12
    dead = ~live
    assert bool((out[dead] == 0).all()) and not bool(torch.signbit(out[dead]).any()) and bool((lse[ref["empty"]] == float("-inf")).all())
    assert bool((ref["out"][dead] == 0).all()) and bool((ref["lse"][ref["empty"]] == float("-inf")).all())


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", PC.DTYPES, ids=_id)
def test_emulation_sits_inside_every_bound(dtype):
    worst = [0.0, 0.0]
    for case in PC.cases():
        r = PC.ratios(*case, dtype, *PC.emulate(*case, dtype))
        assert max(r) <= 1.0, (case, r)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"{_id(dtype)}: worst |d| / bound of the emulation: out {worst[0]:.3f} lse {worst[1]:.3f}")
    assert all(w > 0.0 for w in worst)


@pytest.mark.parametrize("dtype", PC.DTYPES, ids=_id)
@pytest.mark.parametrize("mutant", PC.MUTANTS)
def test_mutants_land_outside_somewhere(mutant, dtype):
    hits = [case for case in SMALL if PC.ratios(*case, dtype, *PC.emulate(*case, dtype, mutant=mutant))[0] > 1.0]
    assert hits, mutant                                                              # outside the bound of OUT, not of lse alone


def test_table_covers_what_it_says():
    cs = PC.cases()
    assert len(cs) == len(PC.SIZES) * len(PC.MASKS) == len(set(cs))
    cols = {"B": [c[0] for c in cs], "heads": [(c[1], c[2]) for c in cs], "size": [c[3:6] for c in cs], "D": [c[6] for c in cs], "mask": [c[7] for c in cs]}
    values = {"B": PC.BATCHES, "heads": PC.HEADS, "size": PC.SIZES, "D": PC.DIMS, "mask": PC.MASKS}
    for a, b in itertools.combinations(cols, 2):                                    # every value of one meets every value of every other
        assert set(zip(cols[a], cols[b])) == set(itertools.product(values[a], values[b])), (a, b)
    assert [s[0] for s in PC.SIZES[:10]] == [1, 2, 31, 32, 33, 255, 256, 257, 515, 1041] and PC.SIZES[10:] == ((5, 38, 33), (257, 768, 255), (3, 552, 0))
    seen = set()
    for case in cs:
        B, Hq, Hkv, Sq, Skv, off, D, mask = case
        if Sq > PC.QB + 1:
            continue                                                                 # the float64 reference of the largest sizes is the GPU test's
        c, ref = PC.make_case(*case, torch.bfloat16), PC.reference(*case, torch.bfloat16)
        lay = PC.layout(Hq, Sq, Skv, D)
        assert lay["Smax"] > Skv and all(lay[n] % 8 == 0 and lay[n] >= D for n in ("k_ss", "v_ss", "o_sh")) and lay["o_sh"] > D
        assert lay["o_ss"] >= Hq * lay["o_sh"] and lay["o_ss"] % 8 == 0
        key = torch.ones(B, Skv, dtype=torch.bool) if c["mask"] is None else c["mask"].clone()
        key[:, off + Sq:] = False
        dead = ~key[:, None, :, None].expand_as(c["k"])
        assert torch.isfinite(c["k"][~dead]).all() and torch.isfinite(c["v"][~dead]).all() and torch.isfinite(c["q"]).all()
        assert not torch.isfinite(c["k"][dead]).any() and not torch.isfinite(c["v"][dead]).any()
        att = PC.attended(c["mask"], B, Sq, Skv, off)
        assert torch.equal(ref["empty"], ~att.any(2)[:, None].expand(B, Hq, Sq))
        if mask == "row_masked":
            assert ref["empty"][B - 1].all() and bool((ref["out"][B - 1] == 0).all()) and bool((ref["lse"][B - 1] == float("-inf")).all())
        if mask == "left_pad" and B == 3 and Sq > 70:
            assert ref["empty"][2, :, :67].all() and not ref["empty"][2, :, 67:].any()      # left-pad query rows are rows without a key
        if mask == "mid_tile" and Skv >= 3 * PC.KT:
            t = ((Skv + PC.KT - 1) // PC.KT) // 2
            assert not c["mask"][:, t * PC.KT:(t + 1) * PC.KT].any() and c["mask"][:, :t * PC.KT].all()
        if mask == "first_qb" and off + Sq > PC.QB:
            assert not c["mask"][:, :PC.QB].any() and c["mask"][:, PC.QB:].all()
        for b in range(B):
            for h in range(Hq):
                fam = c["family"][b][h]
                live = ~ref["empty"][b, h]
                if not live.any():
                    continue
                seen.add(fam)
                i = int(torch.nonzero(live)[-1])
                n = int(att[b, i].sum())
                if fam == "equal":                                                   # out = the mean of the attended V rows, lse = log count
                    assert abs(ref["lse"][b, h, i].item() - math.log(n)) < 1e-12
                    mean = c["v"][b, h // (Hq // Hkv)][att[b, i]].double().mean(0)
                    assert (ref["out"][b, i, h] - mean).abs().max() < 1e-12
                if fam in ("plus90", "minus90"):
                    assert abs(abs(ref["lse"][b, h, i].item()) - 90) < 12
    assert seen == set(PC.FAMILIES)


# ---- the torch route ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(3, 8, 2, 33, 33, 0, 64, "holes"), (1, 4, 4, 257, 257, 0, 128, "null"), (3, 4, 2, 31, 31, 0, 64, "row_masked"),
                                  (3, 3, 3, 5, 38, 33, 128, "left_pad"), (3, 8, 1, 3, 552, 0, 128, "mid_tile")], ids=str)
@pytest.mark.parametrize("dtype", PC.DTYPES, ids=_id)
def test_torch_route_is_the_definition(case, dtype):
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    c, ref = PC.make_case(*case, dtype), PC.reference(*case, dtype)
    lay = PC.layout(Hq, Sq, Skv, D)
    kbuf = torch.full((B, Hkv, lay["Smax"], lay["k_ss"]), float("nan"), dtype=dtype)           # the static-cache form: views of a longer buffer
    vbuf = torch.full((B, Hkv, lay["Smax"], lay["v_ss"]), float("inf"), dtype=dtype)
    kbuf[:, :, :Skv, :D], vbuf[:, :, :Skv, :D] = c["k"], c["v"]
    mask = None if c["mask"] is None else c["mask"][:, None, None, :]
    q = c["q"].transpose(1, 2).contiguous().transpose(1, 2)                                    # the transposed view transformers hands over
    for hip in (False, None):                                                        # None on CPU tensors: the torch ops
        out, lse = LD.prefill_attention(q, kbuf[:, :, :Skv, :D], vbuf[:, :, :Skv, :D], mask, c["scale"], q_offset=off, hip=hip, want_lse=True)
        assert out.shape == (B, Sq, Hq, D) and out.dtype == dtype and out.is_contiguous() and lse.shape == (B, Hq, Sq)
        assert max(PC.ratios_against(ref, out, lse)) <= 1.0
    assert torch.equal(LD.prefill_attention(q, c["k"], c["v"], mask, c["scale"], q_offset=off), out)
    with pytest.raises(_lib.MraError, match="CUDA"):
        LD.prefill_attention(q, c["k"], c["v"], mask, c["scale"], q_offset=off, hip=True)


def test_python_entry_refuses_malformed_calls():
    q, k = torch.zeros(2, 4, 5, 64), torch.zeros(2, 2, 9, 64)
    with pytest.raises(ValueError, match="expected"):
        LD.prefill_attention(q[:, :, 0], k, k, None, 1.0)
    with pytest.raises(ValueError, match="expected"):
        LD.prefill_attention(q, k, k[:, :, :8], None, 1.0)
    with pytest.raises(ValueError, match="q_offset"):
        LD.prefill_attention(q, k, k, None, 1.0, q_offset=5)
    with pytest.raises(ValueError, match="q_offset"):
        LD.prefill_attention(q, k, k, None, 1.0, q_offset=-1)
    with pytest.raises(ValueError, match="key_mask"):
        LD.prefill_attention(q, k, k, torch.ones(2, 1, 1, 8, dtype=torch.bool), 1.0)
    with pytest.raises(ValueError, match="key_mask"):
        LD.prefill_attention(q, k, k, torch.ones(2, 1, 5, 9, dtype=torch.bool), 1.0)  # an [Sq, Skv] mask is not this entry's
    with pytest.raises(ValueError, match="key_mask"):
        LD.prefill_attention(q, k, k, torch.zeros(2, 1, 1, 9), 1.0)


# ---- the ABI entry without a device -----------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments_before_any_launch_and_writes_nothing():
    lib = _lib.lib()
    n = 1 << 16
    buf = C.create_string_buffer(b"\xa5" * n, n)
    p = (C.addressof(buf) + 15) // 16 * 16
    BF = _lib.MRA_BF16
    nan, inf = float("nan"), float("inf")

    def run(q=p, q_sb=300 * 512, q_sh=64, q_ss=512, k=p, k_sb=4 * 400 * 64, k_sh=400 * 64, k_ss=64, v=p, v_sb=4 * 400 * 64, v_sh=400 * 64, v_ss=64,
            mask=p, mask_sb=400, B=2, Hq=8, Hkv=4, Sq=300, Skv=400, off=100, D=64, dt=BF, scale=0.125, out=p, o_sb=300 * 512, o_ss=512, o_sh=64, lse=p):
        return lib.mra_prefill_attention(q, q_sb, q_sh, q_ss, k, k_sb, k_sh, k_ss, v, v_sb, v_sh, v_ss, mask, mask_sb, B, Hq, Hkv, Sq, Skv, off, D, dt, scale,
                                         out, o_sb, o_ss, o_sh, lse, None)

    bad = [("null", dict(q=None)), ("null", dict(k=None)), ("null", dict(v=None)), ("null", dict(out=None)),
           ("multiple of Hkv", dict(Hq=7)), ("multiple of Hkv", dict(Hkv=0)), ("1, 2, 4 or 8", dict(Hq=12)), ("1, 2, 4 or 8", dict(Hq=64)),
           ("D must", dict(D=32)), ("D must", dict(D=96)), ("D must", dict(D=256)), ("at least 1", dict(Sq=0)), ("at least 1", dict(Skv=0, Sq=1, off=0)),
           ("q_offset", dict(off=-1)), ("q_offset", dict(off=101)), ("q_offset", dict(Sq=401, off=0)), ("negative B", dict(B=-1)),
           ("at most 65535", dict(B=65536)), ("at most 65535", dict(Hkv=65536, Hq=65536)), ("2^30", dict(Skv=(1 << 30) + 1)),
           ("dtype", dict(dt=_lib.MRA_F32)), ("dtype", dict(dt=9)),
           ("16-byte aligned", dict(q=p + 8)), ("16-byte aligned", dict(k=p + 2)), ("16-byte aligned", dict(v=p + 4)), ("16-byte aligned", dict(out=p + 8)),
           ("4-byte aligned", dict(lse=p + 2)),
           ("strides", dict(q_sb=516)), ("strides", dict(q_sh=68)), ("strides", dict(q_ss=513)), ("strides", dict(k_sb=4)), ("strides", dict(k_sh=400 * 64 + 1)),
           ("strides", dict(k_ss=68)), ("strides", dict(v_sb=12)), ("strides", dict(v_sh=7)), ("strides", dict(v_ss=100)), ("strides", dict(o_sb=514)),
           ("strides", dict(o_ss=516)), ("strides", dict(o_sh=66)),
           ("below D", dict(q_ss=56)), ("below D", dict(k_ss=56)), ("below D", dict(v_ss=0)), ("below D", dict(k_ss=-64)), ("below D", dict(o_ss=8)),
           ("below D", dict(o_sh=0)),
           ("scale", dict(scale=nan)), ("scale", dict(scale=inf)), ("scale", dict(scale=-inf))]
    for msg, kw in bad:
        assert run(**kw) == -1, kw
        assert msg.encode() in lib.mra_last_error(), (kw, lib.mra_last_error())
        assert buf.raw == b"\xa5" * n, kw                                            # nothing was written
    # B == 0 launches nothing and needs nothing, not even pointers
    assert run(B=0, q=None, k=None, v=None, out=None) == 0
    assert buf.raw == b"\xa5" * n
