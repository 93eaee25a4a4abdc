"""CPU: the case table of tests/raw_scores_cases.py (the scores launch of the folded cross-attention over raw encoder tokens) against its own
float64 references -- the fp32 emulation of the launch stays inside every bound, the bar on the token factors r_n is the emulation's error
with its stated margin and lies where the analysis puts it, and the E[x^2] - mean^2 formulation the kernel avoids misses that bar on the
same rows.  No GPU, no library call."""
import pytest
import torch

import raw_scores_cases as R


def test_table_covers_the_shapes_the_launch_differs_in():
    seen = {(c["M"], c["N"], c["K"], c["kind"]) for c in R.CASES}
    assert len(seen) == len(R.CASES) == 16
    for c in R.CASES:
        assert c["batch"] == 2 and c["K"] % 64 == 0
        assert (c["N"] % R.TILE == 0) == (c["N"] == 176)            # one exact tile, or a full tile plus a ragged one of 40
        assert R.ntiles(c) == (1 if c["N"] == 176 else 2)
    assert {c["K"] // 64 for c in R.CASES} == {2, 3}                 # both LDS buffers as the last one; an odd count
    d = R.inputs(R.CASES[0]["name"], "f16")
    W = d["W"].double()
    assert W.mean(-1).min() < -5.5 and W.mean(-1).max() > 5.5
    assert W.std(-1).min() < 0.08 and W.std(-1).max() > 6.0
    assert (W.mean(-1).abs() / W.std(-1)).max() > 30                 # |mean| >> sigma on some rows


def test_the_bar_on_r_is_the_emulation_error_with_its_margin():
    bar = R.r_bar("f16")
    worst_emu, worst_case = 0.0, 0.0
    for c in R.CASES:
        d, ref = R.inputs(c["name"], "f16"), R.reference(c["name"], "f16")
        emu = torch.stack([R.r_emulate(d["W"][b]) for b in range(c["batch"])])
        worst_emu = max(worst_emu, R.r_error(ref, emu))
        # first-order worst case of the merge order (raw_scores_cases docstring) on the worst row
        sig = ref["var"].sqrt()
        worst_case = max(worst_case, float((16 * R.U32 * (ref["mean"].abs() + 4 * sig) / sig).max()))
    print(f"r: emulation {worst_emu / R.U32:.1f} u32, bar {bar / R.U32:.1f} u32, first-order worst case {worst_case / R.U32:.0f} u32")
    assert worst_emu * R.R_MARGIN == pytest.approx(bar)
    assert 4 * R.U32 < bar < worst_case


def test_mean_of_squares_minus_square_of_mean_misses_the_bar():
    bar = R.r_bar("f16")
    for c in R.CASES[::4]:
        d, ref = R.inputs(c["name"], "f16"), R.reference(c["name"], "f16")
        naive = torch.stack([R.r_naive(d["W"][b]) for b in range(c["batch"])])
        err = ((naive.double() - ref["r"]).abs() / ref["r"]).nan_to_num(nan=float("inf"))
        print(f"{c['name']}: E[x^2] - mean^2 in fp32 errs by {float(err.max()) / R.U32:.0f} u32 (bar {bar / R.U32:.1f} u32)")
        assert float(err.max()) > 50 * bar


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("name", [c["name"] for c in R.CASES[::3]])
def test_emulated_launch_is_inside_every_bound(name, dt):
    ratios, fails = R.check(name, dt, R.emulate(name, dt))
    print(name, dt, ratios)
    assert not fails, fails


def test_check_catches_what_it_should():
    name = "m200_kv216_k192_peaked"
    c, ref = R.BY_NAME[name], R.reference(name, "f16")
    good = R.emulate(name, "f16")
    # the factor left out of C; stat_l summed over what is stored; the ragged tail in the sum; r from the naive formulation
    o = {k: v.clone() for k, v in good.items()}
    o["C"] = R.emulate(name, "f16", r=torch.ones(c["batch"], c["N"]))["C"]
    assert any(f.startswith("C") for f in R.check(name, "f16", o)[1])
    o = {k: v.clone() for k, v in good.items()}
    B, M, ld, nt = c["batch"], c["M"], R.fold_kvp(c["N"]), R.ntiles(c)
    o["stat_l"][:B * M * nt] = good["C"].view(B, M, ld)[:, :, :nt * R.TILE].float().view(B, M, nt, R.TILE).sum(-1).reshape(-1)
    assert any(f.startswith("stat_l") for f in R.check(name, "f16", o)[1])
    o = {k: v.clone() for k, v in good.items()}
    o["C"].view(B, M, ld)[:, :, c["N"]:nt * R.TILE] = 1e-3
    assert any(f.startswith("C") for f in R.check(name, "f16", o)[1])
    naive = torch.stack([R.r_naive(R.inputs(name, "f16")["W"][b]) for b in range(B)]).nan_to_num(nan=1.0, posinf=1.0)
    assert any(f.startswith("r") for f in R.check(name, "f16", R.emulate(name, "f16", r=naive))[1])
    o = {k: v.clone() for k, v in good.items()}
    o["col_scale"][c["N"]] = 1.0          # a column past N written
    assert any("outside" in f for f in R.check(name, "f16", o)[1])
