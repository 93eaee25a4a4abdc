"""The backward of the prefill attention without a GPU (``-m "not gpu"``): the float64 reference of tests/prefill_bwd_cases.py equals
torch.autograd over ``lm_decode._torch_ops``; the fp32 emulation of csrc/prefill_attn_bwd.hip sits inside the derived bounds and every named
mutant lands outside; the table covers what it says; ``causal_attention`` on the CPU is the definition under autograd; the entry refuses bad
arguments with host pointers before any launch and writes nothing; the workspace formula."""
import ctypes as C
import itertools
import os
import re

import pytest
import torch

import prefill_bwd_cases as BC
from mraudio_amd import _lib
from mraudio_amd.models import lm_attention as LA
from mraudio_amd.models import lm_decode as LD

SMALL = [c for c in BC.cases() if c[3] <= BC.KB + 1]             # the mutants are run where a case takes milliseconds


def _id(dt):
    return str(dt).split(".")[-1]


def test_constants_are_the_kernels():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mraudio_amd", "csrc", "kernels.h")).read()
    m = re.search(r"constexpr int PREFILL_BWD_QB = (\d+), PREFILL_BWD_KB = (\d+), PREFILL_BWD_QT = (\d+)", text)
    assert m and tuple(int(g) for g in m.groups()) == (BC.QB, BC.KB, BC.QT)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in BC.cases() if c[3] in (2, 33, BC.KB + 1, 5, 3)], ids=str)
def test_float64_reference_is_autograd_over_the_torch_ops(case):
    B, Hq, Hkv, Sq, Skv, off, D, _ = case
    c = BC.make_case(*case, torch.bfloat16)
    f = BC._forward64(c["q"], c["k"], c["v"], c["mask"], c["scale"], off)
    ref = BC.reference_tensors(c["q"], c["k"], c["v"], c["mask"], c["dout"], f["out"].transpose(1, 2), f["lse"], c["scale"], off, torch.bfloat16)
    q, k, v = (t.double().nan_to_num(0, 0, 0).requires_grad_(True) for t in (c["q"], c["k"], c["v"]))
    km = None if c["mask"] is None else c["mask"][:, None, None, :]
    out, lse = LD._torch_ops(q, k, v, km, c["scale"], off)                             # [B, Hq, Sq, D]
    live = ~ref["empty"]
    assert torch.equal(live, lse > float("-inf"))
    dout = torch.where(live[..., None], c["dout"].double().transpose(1, 2), torch.zeros((), dtype=torch.float64))
    out.backward(dout)
    assert live.any() or case[7] == "row_masked"
    for name, g in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        assert bool(torch.isfinite(g).all())
        rows = live if name == "dq" else ~ref["dead"][:, None, :].expand(B, Hkv, Skv)
        if rows.any():
            # 1e-12 of max(1, |value|): under the plus90 / minus90 families dK reaches 6e2 and its terms (q_0 = +-180) cancel, so a few
            # float64 ulps of these sums are 3e-12; a tighter relative figure fails on an element of 7.1 whose terms are that large
            assert bool(((g[rows] - ref[name][rows]).abs() <= 1e-12 * ref[name][rows].abs().clamp(min=1.0)).all()), name
        assert bool((g[~rows] == 0).all()) and bool((ref[name][~rows] == 0).all()) and not bool(torch.signbit(ref[name][~rows]).any())
    # causal_attention on CPU tensors is that route: one call, the same gradients, out as [B, Sq, Hq, D]
    q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o2 = LA.causal_attention(q2, k2, v2, km, c["scale"], q_offset=off)
    assert o2.shape == (B, Sq, Hq, D) and torch.equal(o2, out.transpose(1, 2))
    o2.backward(dout.transpose(1, 2))
    assert torch.equal(q2.grad, q.grad) and torch.equal(k2.grad, k.grad) and torch.equal(v2.grad, v.grad)
    with torch.no_grad():
        assert torch.equal(LA.causal_attention(q2, k2, v2, km, c["scale"], q_offset=off), LD.prefill_attention(q2, k2, v2, km, c["scale"], q_offset=off))
    with pytest.raises(_lib.MraError, match="CUDA"):
        LA.causal_attention(q2, k2, v2, km, c["scale"], q_offset=off, hip=True)


# ---- the table ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", BC.DTYPES, ids=_id)
def test_emulation_sits_inside_every_bound(dtype):
    worst = [0.0, 0.0, 0.0]
    for case in BC.cases():
        r = BC.ratios(*case, dtype, *BC.emulate(*case, dtype))
        assert max(r) <= 1.0, (case, r)
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"{_id(dtype)}: worst |d| / bound of the emulation: dq {worst[0]:.3f} dk {worst[1]:.3f} dv {worst[2]:.3f}")
    assert all(w > 0.0 for w in worst)


@pytest.mark.parametrize("dtype", BC.DTYPES, ids=_id)
@pytest.mark.parametrize("mutant", BC.MUTANTS)
def test_mutants_land_outside_somewhere(mutant, dtype):
    assert any(max(BC.ratios(*case, dtype, *BC.emulate(*case, dtype, mutant=mutant))) > 1.0 for case in SMALL), mutant


def test_table_covers_what_it_says():
    cs = BC.cases()
    assert len(cs) == len(BC.SIZES) * len(BC.MASKS) == len(set(cs))
    cols = {"B": [c[0] for c in cs], "heads": [(c[1], c[2]) for c in cs], "size": [c[3:6] for c in cs], "D": [c[6] for c in cs], "mask": [c[7] for c in cs]}
    values = {"B": BC.BATCHES, "heads": BC.HEADS, "size": BC.SIZES, "D": BC.DIMS, "mask": BC.MASKS}
    for a, b in itertools.combinations(cols, 2):                                    # every value of one meets every value of every other
        assert set(zip(cols[a], cols[b])) == set(itertools.product(values[a], values[b])), (a, b)
    assert [s[0] for s in BC.SIZES[:10]] == [1, 2, 31, 32, 33, 127, 128, 129, 259, 1041] and BC.SIZES[10:] == ((5, 38, 33), (129, 384, 127), (3, 296, 0))
    seen = set()
    for case in cs:
        B, Hq, Hkv, Sq, Skv, off, D, mask = case
        if Sq > BC.KB + 1:
            continue
        c, ref = BC.make_case(*case, torch.bfloat16), BC.reference(*case, torch.bfloat16)
        assert torch.isfinite(c["dout"]).all() and torch.isfinite(c["out"]).all() and c["lse"].dtype == torch.float32
        assert torch.equal(ref["empty"], ~(c["lse"] > float("-inf")))
        klive = torch.ones(B, Skv, dtype=torch.bool) if c["mask"] is None else c["mask"].clone()
        klive[:, off + Sq:] = False
        nkb = (Skv + BC.KB - 1) // BC.KB
        blocks = torch.cat([klive, torch.zeros(B, nkb * BC.KB - Skv, dtype=torch.bool)], 1).view(B, nkb, BC.KB).any(2)
        if not blocks.all():
            seen.add("dead key block")
        if ref["empty"].any() and not ref["empty"].all():
            seen.add("dead rows among live ones")
        if ref["dead"].any() and mask in ("holes", "mid_tile"):
            seen.add("masked key under live rows")
        if Hq // Hkv > 1:
            seen.add("group sum")
        if off:
            seen.add("offset")
    assert seen == {"dead key block", "dead rows among live ones", "masked key under live rows", "group sum", "offset"}


def test_workspace_formula():
    lib = _lib.lib()
    for B, Hq, Sq in ((1, 1, 1), (3, 8, 1041), (2, 32, 5400), (0, 4, 9), (7, 3, 63)):
        assert int(lib.mra_prefill_attention_backward_workspace_bytes(B, Hq, Sq)) == BC.workspace_bytes(B, Hq, Sq) >= 4 * B * Hq * Sq
    for bad in ((-1, 4, 9), (1, 0, 9), (1, 4, 0)):
        assert int(lib.mra_prefill_attention_backward_workspace_bytes(*bad)) == 0 and b"workspace_bytes" in lib.mra_last_error()


# ---- the ABI entry without a device -----------------------------------------------------------------------------------------------------------
def test_entry_refuses_bad_arguments_before_any_launch_and_writes_nothing():
    lib = _lib.lib()
    n = 1 << 16
    buf = C.create_string_buffer(b"\xa5" * n, n)
    p = (C.addressof(buf) + 15) // 16 * 16
    BF = _lib.MRA_BF16
    nan, inf = float("nan"), float("inf")
    need = BC.workspace_bytes(2, 8, 300)

    def run(q=p, q_sb=300 * 512, q_sh=64, q_ss=512, k=p, k_sb=4 * 400 * 64, k_sh=400 * 64, k_ss=64, v=p, v_sb=4 * 400 * 64, v_sh=400 * 64, v_ss=64,
            mask=p, mask_sb=400, out=p, o_sb=300 * 512, o_ss=512, o_sh=64, dout=p, do_sb=300 * 512, do_ss=512, do_sh=64, lse=p, B=2, Hq=8, Hkv=4, Sq=300,
            Skv=400, off=100, D=64, dt=BF, scale=0.125, dq=p, dq_sb=300 * 512, dq_sh=64, dq_ss=512, dk=p, dk_sb=4 * 400 * 64, dk_sh=400 * 64, dk_ss=64,
            dv=p, dv_sb=4 * 400 * 64, dv_sh=400 * 64, dv_ss=64, ws=p, ws_bytes=need):
        return lib.mra_prefill_attention_backward(q, q_sb, q_sh, q_ss, k, k_sb, k_sh, k_ss, v, v_sb, v_sh, v_ss, mask, mask_sb, out, o_sb, o_ss, o_sh, dout,
                                                  do_sb, do_ss, do_sh, lse, B, Hq, Hkv, Sq, Skv, off, D, dt, scale, dq, dq_sb, dq_sh, dq_ss, dk, dk_sb,
                                                  dk_sh, dk_ss, dv, dv_sb, dv_sh, dv_ss, ws, ws_bytes, None)

    bad = [("null", dict(**{name: None})) for name in ("q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "ws")]
    bad += [("16-byte aligned", dict(**{name: p + 8})) for name in ("q", "k", "v", "out", "dout", "dq", "dk", "dv", "ws")]
    bad += [("4-byte aligned", dict(lse=p + 2))]
    bad += [("strides", dict(**{name: val})) for name, val in (
        ("q_sb", 516), ("q_sh", 68), ("q_ss", 513), ("k_sb", 4), ("k_sh", 400 * 64 + 1), ("k_ss", 68), ("v_sb", 12), ("v_sh", 7), ("v_ss", 100),
        ("o_sb", 514), ("o_ss", 516), ("o_sh", 66), ("do_sb", 2), ("do_ss", 515), ("do_sh", 65), ("dq_sb", 6), ("dq_sh", 63), ("dq_ss", 519),
        ("dk_sb", 1), ("dk_sh", 3), ("dk_ss", 65), ("dv_sb", 5), ("dv_sh", 9), ("dv_ss", 70))]
    bad += [("below D", dict(**{name: val})) for name, val in (
        ("q_ss", 56), ("k_ss", 56), ("v_ss", 0), ("k_ss", -64), ("o_ss", 8), ("o_sh", 0), ("do_ss", 56), ("do_sh", 8), ("dq_ss", 56), ("dk_ss", 32), ("dv_ss", 0))]
    bad += [("multiple of Hkv", dict(Hq=7)), ("multiple of Hkv", dict(Hkv=0)), ("1, 2, 4 or 8", dict(Hq=12)), ("1, 2, 4 or 8", dict(Hq=64)),
            ("D must", dict(D=32)), ("D must", dict(D=96)), ("D must", dict(D=256)), ("at least 1", dict(Sq=0)), ("at least 1", dict(Skv=0, Sq=1, off=0)),
            ("q_offset", dict(off=-1)), ("q_offset", dict(off=101)), ("q_offset", dict(Sq=401, off=0)), ("negative B", dict(B=-1)),
            ("at most 65535", dict(B=65536, ws_bytes=1 << 40)), ("at most 65535", dict(Hkv=65536, Hq=65536, ws_bytes=1 << 40)),
            ("key blocks", dict(Skv=65535 * BC.KB + 1)),
            ("dtype", dict(dt=_lib.MRA_F32)), ("dtype", dict(dt=9)),
            ("workspace too small", dict(ws_bytes=need - 1)), ("workspace too small", dict(ws_bytes=0)),
            ("scale", dict(scale=nan)), ("scale", dict(scale=inf)), ("scale", dict(scale=-inf))]
    for msg, kw in bad:
        assert run(**kw) == -1, kw
        assert msg.encode() in lib.mra_last_error(), (kw, lib.mra_last_error())
        assert buf.raw == b"\xa5" * n, kw                                            # nothing was written
    # B == 0 launches nothing and needs nothing, not even pointers
    assert run(B=0, q=None, k=None, v=None, out=None, dout=None, lse=None, dq=None, dk=None, dv=None, ws=None, ws_bytes=0) == 0
    assert buf.raw == b"\xa5" * n
