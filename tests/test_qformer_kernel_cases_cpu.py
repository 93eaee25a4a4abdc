"""No GPU: what tests/test_gpu_qformer_kernels.py rests on before a kernel runs -- every bound of ``tests/qformer_kernel_cases.py`` against
the fp32 emulation of the kernel it covers (the faithful emulation inside, each named mutant outside on at least one family), the
assumptions the input builders make (constant rows are exact, histogram inputs are clear of bin edges, what the (hi, lo) split keeps),
and the argument checks of the new ``mra_debug_*`` entries that need no device."""
import ctypes as C

import pytest
import torch

import qformer_kernel_cases as K
from mraudio_amd import _lib

DTYPES = (torch.float16, torch.bfloat16)
ITEMS, HEADS = 3, 2
CPU_S = (33, 65, 225)     # a partial query block and tile; three tiles; 8 tiles (the four-wave kernel's threshold)


# ---- self-attention -------------------------------------------------------------------------------------------------------------------
def _attn_ratios(kind, S, dtype, mask_kind, mutant=None):
    q, k, v = K.make_attn(kind, ITEMS, HEADS, S, dtype)
    mask = K.make_mask(mask_kind, ITEMS, S)
    ref, bound, lse_ref, lse_bound = K.attn_ref(q, k, v, mask)
    out, lse = K.attn_emulate(q, k, v, mask, mutant=mutant)
    return K.worst_ratio(out, ref, bound), K.worst_ratio(lse, lse_ref, lse_bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", CPU_S)
def test_emulated_self_attention_sits_inside_the_bounds(S, dtype):
    worst = (0.0, None)
    worst_lse = (0.0, None)
    for kind in K.ATTN_FAMILIES:
        for mk in K.MASK_KINDS:
            r, rl = _attn_ratios(kind, S, dtype, mk)
            worst, worst_lse = max(worst, (r, (kind, mk))), max(worst_lse, (rl, (kind, mk)))
    print(f"self-attention emulation S={S} {dtype}: ctx / bound {worst[0]:.3f} at {worst[1]}, lse / bound {worst_lse[0]:.3f} at {worst_lse[1]}")
    assert worst[0] <= 0.5 and worst_lse[0] <= 0.5, (worst, worst_lse)   # above half: the bound does not fit this kernel -- do not widen it


def test_the_all_zero_mask_row_cancels_in_the_reference_and_shows_in_fp32():
    """The reference of an all-zero mask row is the unmasked softmax; in fp32 the -14427 costs score bits (the row's error grows against
    the same row run without a mask) and the row stays inside the bound with its z term."""
    S, dtype = 65, torch.float16
    grew = 0
    for kind in K.ATTN_FAMILIES:
        q, k, v = K.make_attn(kind, ITEMS, HEADS, S, dtype)
        mask = K.make_mask("zero_row", ITEMS, S)
        ref, bound, _, _ = K.attn_ref(q, k, v, mask)
        out, _ = K.attn_emulate(q, k, v, mask)
        unmasked, _ = K.attn_emulate(q, k, v, None)
        assert torch.allclose(ref[1], K.attn_ref(q, k, v, None)[0][1], rtol=0, atol=1e-9), "the -10000 does not cancel in the reference"
        assert K.worst_ratio(out[1], ref[1], bound[1]) <= 1.0
        grew += (out[1].double() - ref[1]).abs().mean().item() > (unmasked[1].double() - ref[1]).abs().mean().item()
    assert grew >= 3, grew
    assert abs(K.ZERO_ROW_REL - 2 * 2.0 ** -11 * 0.6931471805599453) < 1e-6


ATTN_MUTANT_CASES = {
    # mutant: (family, S, mask kind, which output) -- the family asserted; others may catch it too
    "mask_last_tile": ("mild", 65, "ragged", "ctx"),
    "tail": ("mild", 33, "ones", "ctx"),
    "alpha": ("onehot_last", 65, "null", "ctx"),
    "qclamp": ("mild", 33, "null", "ctx"),
    "lse_ln": ("mild", 33, "null", "lse"),
}


@pytest.mark.parametrize("mutant", K.ATTN_MUTANTS)
def test_attention_mutants_leave_the_bound(mutant):
    kind, S, mk, which = ATTN_MUTANT_CASES[mutant]
    r, rl = _attn_ratios(kind, S, torch.float16, mk, mutant=mutant)
    got = r if which == "ctx" else rl
    print(f"mutant {mutant}: {which} / bound = {got:.1f} on {kind} S={S} mask={mk}")
    assert got > 1.0


# ---- LayerNorm family -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", K.LN_H)
def test_emulated_layernorm_sits_inside_the_bound(H):
    (g, b), = K.make_ln_params(1, H)
    worst = (0.0, None)
    for kind in K.LN_FAMILIES:
        for eps in (1e-12, 1e-5):
            x = K.make_ln_rows(kind, 8, H)
            ref, bound = K.ln_ref(x, g.expand_as(x), b.expand_as(x), eps)
            for div in (False, True):
                y = K.ln_emulate(x, g, b, eps, by_division=div)
                worst = max(worst, (K.worst_ratio(y, ref, bound), (kind, eps, div)))
                if kind == "constant":
                    assert torch.equal(y, b.expand_as(x)), (H, eps, div)
    print(f"layernorm emulation H={H}: y32 / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 0.5, worst


def test_constant_rows_have_an_exact_fp32_mean():
    assert all(K.constant_rows_are_exact(H, by_division=False) for H in K.LN_H)
    assert all(K.constant_rows_are_exact(E, by_division=True) for E in K.MODALITY_E)


def test_one_pass_variance_leaves_the_bound_on_the_offset_families():
    H = 768
    (g, b), = K.make_ln_params(1, H)
    seen = {}
    for kind in K.LN_FAMILIES:
        x = K.make_ln_rows(kind, 8, H)
        ref, bound = K.ln_ref(x, g.expand_as(x), b.expand_as(x), 1e-12)
        seen[kind] = K.worst_ratio(K.ln_emulate(x, g, b, 1e-12, mutant="one_pass"), ref, bound)
    print("mutant one_pass: y32 / bound " + ", ".join(f"{k} {v:.2f}" for k, v in seen.items()))
    assert seen["offset1000"] > 1.0 and seen["offset50_small"] > 1.0


def test_a_wrong_parameter_set_on_one_row_class_is_gross():
    H, S, N = 256, 37, 2
    sets = K.make_ln_params(4, H)
    rows = 2 * N * S
    idx = K.ln_set_index(rows, S, 32, N * S, True, True)
    assert idx.tolist()[:S] == [0] * 32 + [1] * 5 and idx.tolist()[N * S:N * S + S] == [2] * 32 + [3] * 5
    assert K.ln_set_index(rows, S, 32, N * S, True, False).tolist()[N * S:N * S + S] == [2] * S     # gain4 == NULL: set 3 for all rows
    x = K.make_ln_rows("normal", rows, H)
    G, B = torch.stack([s[0] for s in sets])[idx], torch.stack([s[1] for s in sets])[idx]
    ref, bound = K.ln_ref(x, G, B, 1e-12)
    assert K.worst_ratio(K.ln_emulate(x, G, B, 1e-12), ref, bound) <= 0.5
    wrong = idx.clone()
    wrong[N * S + 32:N * S + S] = 2     # mutant wrong_set: the text rows of the second lane take set 3 instead of set 4
    r = K.worst_ratio(K.ln_emulate(x, torch.stack([s[0] for s in sets])[wrong], torch.stack([s[1] for s in sets])[wrong], 1e-12), ref, bound)
    print(f"mutant wrong_set: y32 / bound = {r:.0f}")
    assert r > 1e3


def test_embedding_rows_before_the_layernorm():
    ids, query, word, pos = K.make_embed(3, 5, 256, 11, per_item_query=False)
    assert ids.min() < 0 and ids.max() >= 11 and (ids == 0).any() and (ids == 10).any()
    pre = K.embed_pre(ids, query, word, pos, 3, 5)
    assert pre.shape == (3, 37, 256) and torch.equal(pre[2, :32], query[0]) and torch.equal(pre[1, 32], word[ids[1, 0].clamp(0, 10)] + pos[0])
    assert K.embed_pre(ids[:, :0], query, word, pos, 3, 0).shape == (3, 32, 256)


# ---- folded-attention helpers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_emulated_softmax_rows_sit_inside_the_bound(dtype):
    worst = (-1.0, None)
    for kvp in (4, 1028, 4100):
        for kv in sorted({kvp, kvp - 3, 1}):
            for kind in ("mild", "peaked"):
                s = K.make_scores(kind, 5, kv, kvp + 8)
                ref, bound = K.softmax_ref(s, kv, kvp, 0.125, dtype)
                out = K.softmax_emulate(s, kv, kvp, 0.125, dtype)
                assert (out[:, kv:] == 0).all()
                worst = max(worst, (K.worst_ratio(out[:, :kv], ref[:, :kv], bound[:, :kv]), (kvp, kv, kind)))
    print(f"softmax_rows emulation {dtype}: P / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst     # the one rounding of P to T alone reaches u p, the leading term of the bound


def test_softmax_mutant_that_counts_the_padding_leaves_the_bound():
    kv, kvp = 1025, 1028
    s = K.make_scores("mild", 5, kv, kvp + 8)
    ref, bound = K.softmax_ref(s, kv, kvp, 0.125, torch.float16)
    out = K.softmax_emulate(s, kv, kvp, 0.125, torch.float16, mutant="tail_counted")
    r = K.worst_ratio(out[:, :kv], ref[:, :kv], bound[:, :kv])
    print(f"mutant tail_counted: P / bound = {r:.1f}; padding columns non-zero: {bool((out[:, kv:] != 0).any())}")
    assert r > 1.0 and (out[:, kv:] != 0).any()


@pytest.mark.parametrize("ntiles", (1, 2, 12, 64, 65, 128))
def test_emulated_row_factors_sit_inside_the_bound_and_histogram_inputs_are_safe(ntiles):
    m, l, pt = K.make_tile_stats(64, ntiles, 8, torch.float16)
    assert K.hist_is_safe(m, l).all()
    g_ref, g_bound, inv = K.factor_ref(m, l)
    if ntiles > 1:
        assert (g_ref.amin(-1) < 2.0 ** -126).all(), "no tile of the row underflows"
    assert K.hist_ref(m, l).sum().item() == 64 and (inv > 0).all() and (inv <= 1.0 + 1e-12).all()
    assert (K.hist_ref(m, l) > 0).sum().item() >= 4, "the rows land in too few bins to test the histogram"
    r = K.worst_ratio(K.factor_emulate(m, l), g_ref, g_bound)
    print(f"row factor emulation ntiles={ntiles}: g / bound {r:.3f}")
    assert r <= 1.0
    if ntiles > 1:
        rm = K.worst_ratio(K.factor_emulate(m, l, mutant="first_tile_max"), g_ref, g_bound)
        print(f"mutant first_tile_max ntiles={ntiles}: g / bound = {rm:.3g}")
        assert rm > 1.0


# ---- splitters ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_what_the_hi_lo_pair_keeps(dtype):
    """csrc/norm_embed.hip: "~22 significant bits with f16".  hi + lo is within 2^-22 |x| wherever lo is a normal number of T; below that
    the absolute floor of T's subnormals takes over (f16: |x - (hi + lo)| <= 2^-25 for every finite |x| <= 65504, reached from
    |x| < 2^-3 down) -- DESIGN.md states the measured floor."""
    x = K.make_split_values(4096, dtype).double()
    hi, lo = K.split_ref(x.float(), dtype)
    err = (x - (hi.double() + lo.double())).abs()
    bits = 22 if dtype == torch.float16 else 16
    floor = 2.0 ** -25 if dtype == torch.float16 else 2.0 ** -134
    assert (err <= torch.maximum(x.abs() * 2.0 ** -bits, torch.tensor(floor, dtype=torch.float64))).all()
    rel_fails = (err > x.abs() * 2.0 ** -bits) & (x != 0)
    print(f"{dtype}: hi + lo misses {bits} bits on {int(rel_fails.sum())} of {x.numel()} values, largest |x| among them "
          f"{x.abs()[rel_fails].max().item() if rel_fails.any() else 0.0:.3g}; worst absolute error there {err[rel_fails].max().item() if rel_fails.any() else 0.0:.3g}")
    if dtype == torch.float16:
        assert rel_fails.any() and x.abs()[rel_fails].max().item() < 2.0 ** -3     # the claim fails only for small |x|
    # the layouts
    w = x.float()[:64 * 6].view(64, 6)
    r = K.split_rows_ref(x.float()[:2 * 128].view(2, 128), 64, 3, dtype)
    assert r.shape == (2, 384) and torch.equal(r[:, 0:64], r[:, 128:192]) and torch.equal(r[0, 192:256], hi[64:128])
    assert K.split_weight_ref(w, dtype).shape == (64, 18) and K.split_key_weight_ref(w, 1, dtype).shape == (1, 6, 192)


# ---- scorer ---------------------------------------------------------------------------------------------------------------------------
def test_emulated_scorer_sits_inside_the_bound():
    worst = 0.0
    for H in (4, 260, 768):
        for Q in (1, 7, 32):
            for t_rows in (1, 3):
                z, t = K.make_cosine(3, Q, H, t_rows)
                ref, bound = K.cosine_ref(z, t)
                sim = K.cosine_emulate(z, t)
                assert sim[0, 0].item() == 0.0 and ref[0, 0].item() == 0.0
                if Q > 2:
                    assert abs(ref[0, -1].item() - 1.0) < 1e-12
                if Q > 1:
                    assert abs(ref[0, 1].item() + 1.0) < 1e-12
                if t_rows > 1:
                    assert (sim[-1] == 0).all()
                worst = max(worst, K.worst_ratio(sim, ref, bound))
    print(f"scorer emulation: sim / bound {worst:.3f}")
    assert worst <= 0.5


# ---- the ABI entries without a device -------------------------------------------------------------------------------------------------
def _view(*v):
    return (C.c_int64 * 3)(*v)


def test_debug_entries_reject_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory: every call below must return before it would launch."""
    L = _lib.lib()
    fake = C.create_string_buffer(1 << 16)
    F16, F32 = _lib.MRA_F16, _lib.MRA_F32
    err = L.mra_last_error
    # self-attention
    assert L.mra_debug_self_attention(None, None, F16, 0, 33, 2, None, None, None) == 0            # no items: no-op
    assert L.mra_debug_self_attention(None, None, F16, 2, 33, 2, fake, None, None) == -1 and b"null" in err()
    assert L.mra_debug_self_attention(fake, None, F32, 2, 33, 2, fake, None, None) == -1 and b"dtype" in err()
    assert L.mra_debug_self_attention(fake, None, F16, 2, 0, 2, fake, None, None) == -1
    assert L.mra_debug_self_attention(fake, None, F16, 2, 33, 0, fake, None, None) == -1
    assert L.mra_debug_self_attention(fake, None, F16, -1, 33, 2, fake, None, None) == -1
    # ln_rows
    pp = (C.c_void_p * 8)(*([C.addressof(fake)] * 2 + [None] * 6))
    v = _view(0, 4, 256)
    assert L.mra_debug_ln_rows(None, None, 0, 256, None, 0, 1, 1, 1e-12, None, None, None, None, F16, None) == 0     # no rows: no-op
    assert L.mra_debug_ln_rows(fake, v, 4, 256, pp, 4, 1, 1, 1e-12, None, None, None, None, F16, None) == -1          # no output
    assert L.mra_debug_ln_rows(fake, v, 4, 300, pp, 4, 1, 1, 1e-12, fake, v, None, None, F16, None) == -1 and b"H must" in err()
    assert L.mra_debug_ln_rows(fake, v, 4, 256, pp, 4, 0, 1, 1e-12, fake, v, None, None, F16, None) == -1             # period 0
    assert L.mra_debug_ln_rows(fake, v, 4, 256, pp, 2, 1, 1, 1e-12, fake, v, None, None, F16, None) == -1 and b"set 3" in err()
    assert L.mra_debug_ln_rows(fake, _view(0, 0, 256), 4, 256, pp, 4, 1, 1, 1e-12, fake, v, None, None, F16, None) == -1
    assert L.mra_debug_ln_rows(fake, _view(0, 4, 128), 4, 256, pp, 4, 1, 1, 1e-12, fake, v, None, None, F16, None) == -1 and b"stride" in err()
    assert L.mra_debug_ln_rows(fake, v, 4, 256, None, 4, 1, 1, 1e-12, fake, v, None, None, F16, None) == -1
    half = (C.c_void_p * 8)(*([C.addressof(fake)] * 3 + [None] * 5))
    assert L.mra_debug_ln_rows(fake, v, 4, 256, half, 4, 1, 1, 1e-12, fake, v, None, None, F16, None) == -1 and b"pair" in err()
    assert L.mra_debug_ln_rows(fake, v, 4, 256, pp, 4, 1, 1, 1e-12, fake, v, None, None, F32, None) == -1
    # embed_ln
    assert L.mra_debug_embed_ln(None, 0, 5, 32, 256, 11, None, 0, None, None, None, None, 1e-12, None, None, None, F16, None) == 0
    assert L.mra_debug_embed_ln(None, 2, 5, 32, 256, 11, fake, 0, fake, fake, fake, fake, 1e-12, fake, fake, None, F16, None) == -1   # ids
    assert L.mra_debug_embed_ln(fake, 2, 5, 32, 256, 11, fake, 0, fake, fake, fake, fake, 1e-12, fake, None, None, F16, None) == -1   # h16
    assert L.mra_debug_embed_ln(fake, 2, 5, 32, 200, 11, fake, 0, fake, fake, fake, fake, 1e-12, fake, fake, None, F16, None) == -1
    assert L.mra_debug_embed_ln(fake, 2, 5, 32, 256, 0, fake, 0, fake, fake, fake, fake, 1e-12, fake, fake, None, F16, None) == -1    # vocab
    assert L.mra_debug_embed_ln(fake, 2, -1, 32, 256, 11, fake, 0, fake, fake, fake, fake, 1e-12, fake, fake, None, F16, None) == -1
    # modality_ln: widths the kernel cannot take
    for E in (12, 4104, 0):
        assert L.mra_debug_modality_ln(fake, F32, None, 2, 3, E, fake, fake, 1e-5, fake, F16, None) == -1 and b"E must" in err()
    assert L.mra_debug_modality_ln(fake, 3, None, 2, 3, 64, fake, fake, 1e-5, fake, F16, None) == -1
    assert L.mra_debug_modality_ln(fake, F32, None, 2, 3, 64, None, fake, 1e-5, fake, F16, None) == -1
    assert L.mra_debug_modality_ln(None, F32, None, 0, 3, 64, None, None, 1e-5, None, F16, None) == 0
    # softmax_rows
    assert L.mra_debug_softmax_rows(None, 8, None, 8, 0, 5, 8, 0.125, F16, None) == 0
    assert L.mra_debug_softmax_rows(fake, 8, fake, 8, 2, 0, 8, 0.125, F16, None) == -1
    assert L.mra_debug_softmax_rows(fake, 8, fake, 8, 2, 5, 6, 0.125, F16, None) == -1        # kvp % 4
    assert L.mra_debug_softmax_rows(fake, 8, fake, 4, 2, 5, 8, 0.125, F16, None) == -1        # ld_p < kvp
    assert L.mra_debug_softmax_rows(fake, 4, fake, 8, 2, 5, 8, 0.125, F16, None) == -1        # ld_s < kv
    assert L.mra_debug_softmax_rows(None, 8, fake, 8, 2, 5, 8, 0.125, F16, None) == -1
    # fold_rowfactor / softmax_rescale
    assert L.mra_debug_fold_rowfactor(None, None, None, 0, 32, 2, None, 24, 8, 24, None, None) == 0
    assert L.mra_debug_fold_rowfactor(fake, fake, fake, 64, 32, 2, None, 24, 8, 24, None, None) == -1
    assert L.mra_debug_fold_rowfactor(fake, fake, fake, 64, 513, 2, fake, 24, 8, 24, None, None) == -1
    assert L.mra_debug_fold_rowfactor(fake, fake, fake, 65, 32, 2, fake, 24, 8, 24, None, None) == -1     # rows % R
    assert L.mra_debug_fold_rowfactor(fake, fake, fake, 64, 32, 4, fake, 24, 8, 24, None, None) == -1     # ntiles * tile_cols > kvp
    assert L.mra_debug_fold_rowfactor(fake, fake, fake, 64, 32, 2, fake, 24, 0, 24, None, None) == -1
    assert L.mra_debug_softmax_rescale(None, 24, None, None, 0, 2, 8, 24, F16, None, None) == 0
    assert L.mra_debug_softmax_rescale(fake, 24, fake, fake, 4, 129, 8, 24, F16, None, None) == -1
    assert L.mra_debug_softmax_rescale(fake, 24, fake, fake, 4, 2, 0, 24, F16, None, None) == -1
    assert L.mra_debug_softmax_rescale(fake, 24, fake, fake, 4, 2, 8, 20, F16, None, None) == -1          # kvp % 8
    assert L.mra_debug_softmax_rescale(fake, 16, fake, fake, 4, 2, 8, 24, F16, None, None) == -1          # ld_p < kvp
    assert L.mra_debug_softmax_rescale(fake, 24, None, fake, 4, 2, 8, 24, F16, None, None) == -1
    # transpose_pad
    assert L.mra_debug_transpose_pad(None, None, 0, 40, 40, 0, 0, 1, F16, None) == 0
    assert L.mra_debug_transpose_pad(fake, fake, 41, 40, 40, 41 * 40, 1600, 1, F16, None) == -1           # R > ld_d
    assert L.mra_debug_transpose_pad(fake, fake, 33, 40, 40, 100, 1600, 2, F16, None) == -1 and b"stride" in err()
    assert L.mra_debug_transpose_pad(None, fake, 33, 40, 40, 33 * 40, 1600, 1, F16, None) == -1
    # the 16-byte kernel (C, ld_d multiples of 8 and >= 64) cannot take a batch stride that is no multiple of 8
    assert L.mra_debug_transpose_pad(fake, fake, 61, 64, 64, 61 * 64 + 4, 64 * 64, 2, F16, None) == -1 and b"multiples of 8" in err()
    assert L.mra_debug_transpose_pad(fake, fake, 61, 64, 64, 61 * 64, 64 * 64 + 4, 2, F16, None) == -1
    assert L.mra_debug_transpose_pad(fake, fake, 33, 40, 40, 33 * 40, 1600, 1, F32, None) == -1
    # split
    sv = _view(0, 4, 128)
    assert L.mra_debug_split(0, None, sv, 0, 128, 64, 3, None, F16, None) == 0
    assert L.mra_debug_split(3, fake, sv, 4, 128, 64, 3, fake, F16, None) == -1 and b"kind" in err()
    assert L.mra_debug_split(0, fake, sv, 4, 128, 48, 3, fake, F16, None) == -1                          # C % chunk
    assert L.mra_debug_split(0, fake, sv, 4, 128, 64, 4, fake, F16, None) == -1                          # parts
    assert L.mra_debug_split(0, fake, None, 4, 128, 64, 3, fake, F16, None) == -1                        # no view
    assert L.mra_debug_split(1, fake, None, 4, 0, 0, 0, fake, F16, None) == -1
    assert L.mra_debug_split(2, None, None, 4, 128, 0, 0, fake, F16, None) == -1
    assert L.mra_debug_split(1, fake, None, 4, 128, 0, 0, fake, F32, None) == -1
