"""CPU side of tests/enc_grad_cases.py: every faithful fp32 emulation of the two kernels of csrc/enc_grad.hip sits inside its derived bound at
every shape the GPU test runs, every named mutant sits outside (the ratios are printed), and the three new ABI entries refuse bad arguments
before anything is launched.  A handle cannot be created without a device, so the refusals that need one (a footprint one byte short, a
workspace too small, ``ln.*`` not loaded, training not enabled) are in tests/test_gpu_enc_grad.py."""
import ctypes as C

import pytest
import torch

import enc_grad_cases as EG
from mraudio_amd import _lib


def _id(dtype):
    return str(dtype).split(".")[-1]


# ---- the kvgrad GEMM --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", EG.DTYPES, ids=_id)
@pytest.mark.parametrize("E", EG.ENC_WIDTHS)
def test_kvgrad_emulation_sits_inside_its_bound(E, dtype):
    worst = 0.0
    for layers, Ne, kv in EG.kg_cases():
        dkv, W = EG.make_kvgrad(EG.ncross_of(layers), Ne, kv, E, dtype)
        ref, bound = EG.kvgrad_ref(dkv, W)
        r = EG.ratio(EG.kvgrad_emulate(dkv, W), ref, bound)
        print(f"kvgrad layers {layers} ({Ne}, {kv}) E {E} {_id(dtype)}: ratio {r:.3g}")
        assert r <= 1.0, (layers, Ne, kv, r)
        worst = max(worst, r)
    assert worst > 0.0          # the emulation is fp32: it does not reproduce float64


def test_kvgrad_walk_is_the_token_major_matrix():
    """With values that are exact in fp32 sums (small integers) the address walk of the emulation equals the permuted matrix bit for bit."""
    dkv = torch.randint(-3, 4, (4, 3, EG.HEADS, 40, 64)).to(torch.float16)
    W = torch.randint(-2, 3, (4 * EG.HEADS * 64, 128)).to(torch.float16)
    assert torch.equal(EG.kvgrad_emulate(dkv, W), EG.kvgrad_rows(dkv).float() @ W.float())


KG_MUTANT_SHAPES = {
    "segment_order": [(4, 3, 40), (4, 1, 1), (12, 3, 40)],                  # needs ncross >= 2
    "item_straddle": [(2, 3, 40), (4, 2, 257)],                             # needs a tile that crosses an item
    "tail_rows": [(2, 3, 40), (4, 2, 257), (2, 1, 1)],                      # needs a short last tile
    "last_segment_dropped": [(2, 3, 40), (4, 2, 257), (2, 1, 1), (4, 5, 64)],
}


@pytest.mark.parametrize("dtype", EG.DTYPES, ids=_id)
@pytest.mark.parametrize("mutant", EG.KG_MUTANTS)
def test_kvgrad_mutants_land_outside(mutant, dtype):
    for layers, Ne, kv in KG_MUTANT_SHAPES[mutant]:
        for E in EG.ENC_WIDTHS:
            dkv, W = EG.make_kvgrad(EG.ncross_of(layers), Ne, kv, E, dtype)
            ref, bound = EG.kvgrad_ref(dkv, W)
            r = EG.ratio(EG.kvgrad_emulate(dkv, W, mutant), ref, bound)
            print(f"kvgrad mutant {mutant} layers {layers} ({Ne}, {kv}) E {E} {_id(dtype)}: ratio {r:.3g}")
            assert r > 1.0, (mutant, layers, Ne, kv, E, r)


# ---- the modality LayerNorm backward ----------------------------------------------------------------------------------------------------
X_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@pytest.mark.parametrize("x_dtype", X_DTYPES, ids=_id)
@pytest.mark.parametrize("E", EG.ENC_WIDTHS)
def test_mln_emulation_sits_inside_its_bounds(E, x_dtype):
    for rows in EG.LN_ROWS:
        c = EG.make_mln(rows, E, x_dtype)
        for prefill in (True, False):
            g0, b0 = (c["dgain0"], c["dbias0"]) if prefill else (None, None)
            dx_ref, dx_b, dg_ref, dg_b, db_ref, db_b = EG.mln_ref(c["x"], c["d_out"], c["gain"], g0, b0)
            for inplace in (False, True):
                dx, dg, db = EG.mln_emulate(c["x"], c["d_out"], c["gain"], g0, b0, inplace=inplace)
                rs = (EG.ratio(dx, dx_ref, dx_b), EG.ratio(dg, dg_ref, dg_b), EG.ratio(db, db_ref, db_b))
                print(f"mln rows {rows} E {E} {_id(x_dtype)} prefill {prefill} inplace {inplace}: d_x {rs[0]:.3f} d_gain {rs[1]:.3f} d_bias {rs[2]:.3f}")
                assert max(rs) <= 1.0, (rows, E, prefill, inplace, rs)
        if rows > 1:          # the constant row: xhat is exactly 0, so its d_gain terms vanish and d_x = r (g - mean g)
            dx, _, _ = EG.mln_emulate(c["x"], c["d_out"], c["gain"])
            assert torch.isfinite(dx[-1]).all() and dx[-1].abs().max() > 1.0


def test_mln_reference_is_autograd_of_the_float64_layernorm():
    c = EG.make_mln(5, 768, torch.float32)
    x, g, b = c["x"].double().requires_grad_(True), c["gain"].double().requires_grad_(True), torch.zeros(768, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.layer_norm(x, (768,), g, b, EG.ENC_LN_EPS)
    y.backward(c["d_out"].double())
    dx_ref, _, dg_ref, _, db_ref, _ = EG.mln_ref(c["x"], c["d_out"], c["gain"])
    for got, ref in ((x.grad, dx_ref), (g.grad, dg_ref), (b.grad, db_ref)):
        assert (got - ref).abs().max() <= 1e-9 * ref.abs().max()


@pytest.mark.parametrize("x_dtype", X_DTYPES, ids=_id)
@pytest.mark.parametrize("mutant", EG.LN_MUTANTS)
def test_mln_mutants_land_outside(mutant, x_dtype):
    for E in EG.ENC_WIDTHS:
        for rows in EG.LN_ROWS:
            c = EG.make_mln(rows, E, x_dtype)
            dx_ref, dx_b, dg_ref, dg_b, db_ref, db_b = EG.mln_ref(c["x"], c["d_out"], c["gain"], c["dgain0"], c["dbias0"])
            dx, dg, db = EG.mln_emulate(c["x"], c["d_out"], c["gain"], c["dgain0"], c["dbias0"], inplace=True, mutant=mutant)
            rs = (EG.ratio(dx, dx_ref, dx_b), EG.ratio(dg, dg_ref, dg_b), EG.ratio(db, db_ref, db_b))
            print(f"mln mutant {mutant} rows {rows} E {E} {_id(x_dtype)}: d_x {rs[0]:.3g} d_gain {rs[1]:.3g} d_bias {rs[2]:.3g}")
            hit = {"one_pass_variance": rs[0], "mean_g_dropped": rs[0], "dgain_overwritten": min(rs[1], rs[2]),
                   "inplace_read_after_write": min(rs[1], rs[2])}[mutant]
            assert hit > 1.0, (mutant, rows, E, rs)


# ---- the ABI entries without a device ---------------------------------------------------------------------------------------------------
def test_new_entries_reject_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory; every call below returns before it would launch.  Sizes are checked first, then the
    pointers a non-empty call needs, then the handle -- so each refusal is reached without one."""
    L = _lib.lib()
    f = C.create_string_buffer(1 << 12)
    p = C.addressof(f)
    # mra_qformer_backward_enc(h, enc_items, prompts, L, kv, workspace, workspace_bytes, d_enc, stream)
    assert L.mra_qformer_backward_enc(None, 2, 1, 5, 40, p, 1 << 12, p, None) == -1 and b"null handle" in L.mra_last_error()
    assert L.mra_qformer_backward_enc(None, 2, 0, 5, 40, p, 1 << 12, p, None) == -1 and b"prompts" in L.mra_last_error()
    for bad in ((-1, 1, 5, 40), (2, 1, -1, 40), (2, 1, 5, -1)):
        assert L.mra_qformer_backward_enc(None, *bad, p, 1 << 12, p, None) == -1 and b"negative size" in L.mra_last_error(), bad
    assert L.mra_qformer_backward_enc(None, 2, 1, 5, 40, None, 1 << 12, p, None) == -1 and b"null workspace or d_enc" in L.mra_last_error()
    assert L.mra_qformer_backward_enc(None, 2, 1, 5, 40, p, 1 << 12, None, None) == -1 and b"null workspace or d_enc" in L.mra_last_error()
    # mra_modality_ln_backward(h, x, x_dtype, items, tokens, d_out, d_x, d_gain, d_bias, stream)
    assert L.mra_modality_ln_backward(None, p, _lib.MRA_F16, 2, 3, p, p, p, p, None) == -1 and b"null handle" in L.mra_last_error()
    assert L.mra_modality_ln_backward(None, p, _lib.MRA_F16, -1, 3, p, p, p, p, None) == -1 and b"negative size" in L.mra_last_error()
    assert L.mra_modality_ln_backward(None, p, _lib.MRA_F16, 2, -3, p, p, p, p, None) == -1 and b"negative size" in L.mra_last_error()
    assert L.mra_modality_ln_backward(None, p, 7, 2, 3, p, p, p, p, None) == -1 and b"x_dtype" in L.mra_last_error()
    assert L.mra_modality_ln_backward(None, None, _lib.MRA_F16, 2, 3, p, p, p, p, None) == -1 and b"null x or d_out" in L.mra_last_error()
    assert L.mra_modality_ln_backward(None, p, _lib.MRA_F16, 2, 3, None, p, p, p, None) == -1 and b"null x or d_out" in L.mra_last_error()
    # mra_debug_kvgrad_gemm(h, dkv, dkv_bytes, enc_items, kv, d_enc, d_enc_bytes, stream)
    assert L.mra_debug_kvgrad_gemm(None, p, 1 << 12, 1, 1, p, 1 << 12, None) == -1 and b"null handle" in L.mra_last_error()
    assert L.mra_debug_kvgrad_gemm(None, p, 1 << 12, -1, 1, p, 1 << 12, None) == -1 and b"negative size" in L.mra_last_error()
    assert L.mra_debug_kvgrad_gemm(None, p, 1 << 12, 1, -1, p, 1 << 12, None) == -1 and b"negative size" in L.mra_last_error()
    assert L.mra_debug_kvgrad_gemm(None, None, 1 << 12, 1, 1, p, 1 << 12, None) == -1 and b"null dkv or d_enc" in L.mra_last_error()
    assert L.mra_debug_kvgrad_gemm(None, p, 1 << 12, 1, 1, None, 1 << 12, None) == -1 and b"null dkv or d_enc" in L.mra_last_error()


def test_finetune_takes_train_ln():
    from mraudio_amd.finetune import build_parser

    base = ["--output-dir", "out", "--dataset", "QVH"]
    assert build_parser().parse_args(base).train_ln is False
    assert build_parser().parse_args(base + ["--train-ln"]).train_ln is True
