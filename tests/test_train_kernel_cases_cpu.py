"""No GPU: what tests/test_gpu_train_kernels.py rests on before a kernel runs -- every bound of ``tests/train_kernel_cases.py`` against the
fp32 emulation of the kernel it covers (the faithful emulation inside on every case the GPU test runs, each named mutant outside on at
least one), and the argument checks of the training step's ``mra_debug_*`` entries, which all return before any launch."""
import ctypes as C

import pytest
import torch

import train_kernel_cases as K
from mraudio_amd import _lib

DTYPES = (torch.float16, torch.bfloat16)


# ---- gemm_tn --------------------------------------------------------------------------------------------------------------------------
def _tn_ratios(M, N, K_, dtype, accumulate=True, splits=None, mutant=None, with_db=True):
    y, x, W0, db0 = K.make_tn(M, N, K_, dtype)
    splits = K.tn_splits(M, N, K_) if splits is None else splits
    W0 = W0 if accumulate else None
    db0 = db0 if with_db else None
    dW, bW, db, bb = K.tn_ref(y, x, W0, db0, splits)
    eW, eb = K.tn_emulate(y, x, W0, db0, splits, mutant=mutant)
    return K.ratio(eW, dW, bW), K.ratio(eb, db, bb)


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulated_gemm_tn_sits_inside_the_bound(dtype):
    worst = (0.0, None)
    cases = [(M, 64, 64, True) for M in K.TN_SINGLE_M] + [(257, 64, 64, False), (770, 64, 64, False), (100, 128, 192, True)]
    for M, N, K_, acc in cases:
        worst = max(worst, (max(_tn_ratios(M, N, K_, dtype, acc)), (M, N, K_, acc)))
    for n in (2, 3, 4):       # the groups: one split factor for all jobs
        Ms, Ns, Ks = K.GROUP_M[:n], K.GROUP_N[:n], K.GROUP_K[:n]
        for M, N, K_ in zip(Ms, Ns, Ks):
            worst = max(worst, (max(_tn_ratios(M, N, K_, dtype, splits=K.tn_group_splits(Ms, Ns, Ks))), ("group", n, M)))
    print(f"gemm_tn emulation {dtype}: |d| / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst


def test_the_split_factors_of_the_cases_are_what_the_case_list_says():
    """N = K = 64 is one tile: splits = steps / 4.  257 rows 2 pieces; 531 rows 17 steps in 4 pieces of 5, the last of 2; 645 rows 21 steps in
    5 pieces of 5, the last one step of 5 live rows; 770 rows 25 steps in 6 pieces of 5, the last empty."""
    assert [K.tn_splits(M, 64, 64) for M in (64, 257, 531, 645, 770)] == [1, 2, 4, 5, 6]
    assert (531 + 31) // 32 == 17 and 17 - 3 * 5 == 2
    assert (645 + 31) // 32 == 21 and 21 - 4 * 5 == 1 and 645 - 20 * 32 == 5
    assert (770 + 31) // 32 == 25 and 5 * 5 == 25
    assert K.tn_group_splits(K.GROUP_M, K.GROUP_N, K.GROUP_K) == 1
    assert K.tn_group_splits((300, 257), (64, 64), (64, 64)) == 2


TN_MUTANT_CASES = {"tail_rows": (45, 64, 64), "last_split_dropped": (257, 64, 64), "db_every_block": (100, 128, 192), "prefill_overwritten": (64, 64, 64)}


@pytest.mark.parametrize("mutant", K.TN_MUTANTS)
def test_gemm_tn_mutants_leave_the_bound(mutant):
    for dtype in DTYPES:
        rW, rb = _tn_ratios(*TN_MUTANT_CASES[mutant], dtype, mutant=mutant)
        print(f"gemm_tn {mutant} {dtype}: dW {rW:.3g}, db {rb:.3g}")
        assert max(rW, rb) > 1.0


# ---- ln_bwd ---------------------------------------------------------------------------------------------------------------------------
def _lnb_ratios(kind, rows, H, mutant=None, with_add=True, seed=0):
    c = K.make_lnb(kind, rows, H, seed=seed)
    add = c["add"] if with_add else None
    dx, bx, dg, bg, db, bb = K.lnb_ref(c["x"], c["dy"], c["gamma"], K.LNB_EPS, add, c["dgamma0"], c["dbeta0"])
    ex, eg, eb = K.lnb_emulate(c["x"], c["dy"], c["gamma"], K.LNB_EPS, add, c["dgamma0"], c["dbeta0"], mutant=mutant)
    return K.ratio(ex, dx, bx), K.ratio(eg, dg, bg), K.ratio(eb, db, bb)


@pytest.mark.parametrize("H", K.LNB_H)
def test_emulated_ln_bwd_sits_inside_the_bounds(H):
    worst = [(0.0, None)] * 3
    for rows in K.LNB_ROWS:
        for kind in K.LNB_FAMILIES:
            for with_add in (True, False):
                r = _lnb_ratios(kind, rows, H, with_add=with_add)
                worst = [max(w, (v, (kind, rows, with_add))) for w, v in zip(worst, r)]
    print(f"ln_bwd emulation H={H}: dx {worst[0][0]:.3f} at {worst[0][1]}, dgamma {worst[1][0]:.3f} at {worst[1][1]}, dbeta {worst[2][0]:.3f} at {worst[2][1]}")
    assert max(w[0] for w in worst) <= 1.0, worst


def test_constant_rows_have_xhat_zero_and_rstd_1e6():
    from qformer_kernel_cases import constant_rows_are_exact
    for H in K.LNB_H:
        assert constant_rows_are_exact(H, by_division=False)
        x = K.make_lnb("constant", 5, H)["x"]
        assert K.exact_mean_rows(x).all() and not K.exact_mean_rows(x + 0.1).any() and not K.exact_mean_rows(K.make_lnb("normal", 5, H)["x"]).any()
        assert torch.equal(x - x.sum(-1, keepdim=True) * torch.tensor(1.0 / H, dtype=torch.float32), torch.zeros_like(x))
    c = K.make_lnb("constant", 5, 768)
    x = c["x"]
    assert _lnb_ratios("constant", 5, 768, mutant="no_mean_g")[0] > 1.0      # the bound has teeth on these rows too
    dx, _, dg, _, _, _ = K.lnb_ref(x, c["dy"], c["gamma"], K.LNB_EPS)
    g = c["dy"].double() * c["gamma"].double()
    assert torch.allclose(dx, 1e6 * (g - g.mean(-1, keepdim=True)), rtol=1e-9, atol=0) and dg.abs().max() == 0


LNB_MUTANT_CASES = {"one_pass": ("offset1000", 17, 768), "no_mean_g": ("normal", 5, 256), "dgamma_raw_x": ("offset1000", 16, 1024),
                    "tail_in_dgamma": ("normal", 5, 512)}


@pytest.mark.parametrize("mutant", K.LNB_MUTANTS)
def test_ln_bwd_mutants_leave_the_bound(mutant):
    if mutant == "b_uses_a_gamma":      # two jobs with their own gamma: job b computed with job a's
        a, b = K.make_lnb("normal", 17, 768, seed=1), K.make_lnb("normal", 5, 768, seed=2)
        dx, bx, dg, bg, _, _ = K.lnb_ref(b["x"], b["dy"], b["gamma"], K.LNB_EPS)
        ex, eg, _ = K.lnb_emulate(b["x"], b["dy"], a["gamma"], K.LNB_EPS)
        r = (K.ratio(ex, dx, bx), K.ratio(eg, dg, bg))
    else:
        r = _lnb_ratios(*LNB_MUTANT_CASES[mutant], mutant=mutant)
    print(f"ln_bwd {mutant}: {[f'{v:.3g}' for v in r]}")
    assert max(r) > 1.0
    if mutant in ("dgamma_raw_x", "tail_in_dgamma"):
        assert r[1] > 1.0 and r[0] <= 1.0      # the parameter gradient alone
    if mutant == "tail_in_dgamma":
        assert r[2] > 1.0


# ---- embed_bwd ------------------------------------------------------------------------------------------------------------------------
def _emb_ratios(case, mutant=None):
    items, L, Q, H, vocab = case
    c = K.make_emb(*case)
    dq, bq, dp, bp, dw, bw, hit = K.emb_ref(c["demb"], c["ids"], Q, vocab, c["dquery0"], c["dpos0"], c["dword0"])
    eq, ep, ew = K.emb_emulate(c["demb"], c["ids"], Q, vocab, c["dquery0"], c["dpos0"], c["dword0"], mutant=mutant)
    if mutant is None:
        assert torch.equal(ew[~hit], c["dword0"][~hit])
    return K.ratio(eq, dq, bq), K.ratio(ep, dp, bp), K.ratio(ew, dw, bw)


def test_emulated_embed_bwd_sits_inside_the_bounds_and_the_ids_cover_the_edges():
    for case in K.EMB_CASES:
        r = _emb_ratios(case)
        print(f"embed_bwd emulation {case}: dquery {r[0]:.3f}, dpos {r[1]:.3f}, dword {r[2]:.3f}")
        assert max(r) <= 1.0, (case, r)
    ids = K.make_emb(*K.EMB_CASES[0])["ids"]
    assert (ids == -1).any() and (ids == 10).any() and (ids[:, 0] == 1).all() and (ids[:, -1] == ids[:, -2]).all()
    assert int(K.make_emb(*K.EMB_CASES[1])["ids"][0, 0]) == 5                      # the single id is `vocab`
    assert torch.bincount(K.make_emb(*K.EMB_CASES[2])["ids"].clamp(0, 2).view(-1), minlength=3).min() >= 2     # vocab 3: every row collides


EMB_MUTANT_CASES = {"no_clamp": 0, "pos_off_by_q": 0, "word_overwrite": 2}


@pytest.mark.parametrize("mutant", K.EMB_MUTANTS)
def test_embed_bwd_mutants_leave_the_bound(mutant):
    r = _emb_ratios(K.EMB_CASES[EMB_MUTANT_CASES[mutant]], mutant=mutant)
    print(f"embed_bwd {mutant}: {[f'{v:.3g}' for v in r]}")
    assert max(r) > 1.0


# ---- GELU epilogues -------------------------------------------------------------------------------------------------------------------
GELU_SHAPES = ((70, 128, 192), (133, 256, 128), (293, 512, 192), (293, 512, 128), (70, 256, 64), (64, 128, 192), (27, 128, 192))


def _gelu_ratios(M, N, K_, dtype, with_bias=True, mutant=None):
    A, W, bias, aux_in = K.make_gelu(M, N, K_, dtype, with_bias=with_bias)
    pre, b_aux = K.gelu_both_ref(A, W, bias)
    aux, Cf = K.gelu_both_emulate(A, W, bias, mutant=mutant)
    gref, b_c = K.gelu_of_aux_ref(aux)
    bref, b_b = K.gelu_bwd_ref(A, W, aux_in)
    Cb = K.gelu_bwd_emulate(A, W, aux_in, mutant=mutant)
    return K.ratio(aux, pre, b_aux), K.ratio(Cf, gref, b_c), K.ratio(Cb, bref, b_b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_emulated_gelu_epilogues_sit_inside_the_bounds(dtype):
    worst = [(0.0, None)] * 3
    for shape in GELU_SHAPES:
        for with_bias in (True, False):
            r = _gelu_ratios(*shape, dtype, with_bias=with_bias)
            worst = [max(w, (v, shape)) for w, v in zip(worst, r)]
    print(f"GELU emulation {dtype}: aux {worst[0][0]:.3f}, C of aux {worst[1][0]:.3f}, backward {worst[2][0]:.3f}")
    assert max(w[0] for w in worst) <= 1.0, worst
    A, W, bias, aux = K.make_gelu(70, 128, 192, dtype)
    pre, _ = K.gelu_both_ref(A, W, bias)
    assert pre.abs().max() >= 7.5 and aux.double().abs().max() >= 7.5 and (A.double() @ W.double().T).abs().max() < 8    # |u| = 8 comes from the bias


def test_the_emulated_erf_is_within_the_stated_error_of_erf():
    x = torch.linspace(-6.0, 6.0, 200001)
    assert (K._erf_fast(x).double() - torch.erf(x.double())).abs().max().item() <= K.E_ERF


@pytest.mark.parametrize("mutant", K.GELU_MUTANTS)
def test_gelu_mutants_leave_the_bound(mutant):
    for dtype in DTYPES:
        r = _gelu_ratios(133, 256, 128, dtype, mutant=mutant)
        print(f"GELU {mutant} {dtype}: {[f'{v:.3g}' for v in r]}")
        assert (r[2] if mutant == "no_u_phi" else r[1]) > 1.0


# ---- transpose16_batch ----------------------------------------------------------------------------------------------------------------
def test_emulated_transposes_are_exact_and_the_mutant_is_not():
    used = set()
    for njobs in K.TR_NJOBS:
        shapes = K.tr_shapes(njobs)
        used |= set(shapes)
        srcs = [K.make_tr(R, C_, torch.float16, j) for j, (R, C_) in enumerate(shapes)]
        outs = K.tr_emulate(srcs)
        assert all(torch.equal(o.view(torch.int16), s.view(torch.int16).T) for o, s in zip(outs, srcs))
        bad = K.tr_emulate(srcs, mutant="prev_tiles_x")
        differs = any(not torch.equal(o.view(torch.int16), s.view(torch.int16).T) for o, s in zip(bad, srcs))
        assert differs == (njobs > 1), njobs
    assert used == set(K.TR_SHAPES)


# ---- the ABI entries without a device -------------------------------------------------------------------------------------------------
def test_training_debug_entries_reject_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory: every call below must return before it would launch."""
    L = _lib.lib()
    fake = C.create_string_buffer(1 << 16)
    base = (C.addressof(fake) + 63) & ~63
    F16, F32 = _lib.MRA_F16, _lib.MRA_F32
    err = L.mra_last_error
    P, V, I64, I32 = K.c_ptrs, K.c_views, K.c_i64, K.c_i32

    # gemm_tn_group -----------------------------------------------------------------------------------------------------------------
    def tn(njobs=1, dY=base, X=base, dW=base, db=None, yv=(0, 64, 64), xv=(0, 64, 64), ybs=64, xbs=64, M=40, N=64, K_=64, ldw=64, acc=1, dt=F16):
        n = max(njobs, 1)
        return L.mra_debug_gemm_tn_group(njobs, P([dY] * n), V([yv] * n), I64([ybs] * n), P([X] * n), V([xv] * n), I64([xbs] * n), P([dW] * n),
                                         P([db] * n), I32([M] * n), I32([N] * n), I32([K_] * n), I32([ldw] * n), I32([acc] * n), dt, None)
    assert tn(njobs=0) == -1 and tn(njobs=5) == -1 and b"njobs" in err()
    assert tn(dt=F32) == -1 and b"dtype" in err()
    assert tn(dY=None) == -1 and tn(X=None) == -1 and tn(dW=None) == -1 and b"null" in err()
    assert tn(dY=base + 8) == -1 and b"aligned" in err()
    assert tn(X=base + 2) == -1
    assert tn(yv=(0, 0, 64)) == -1 and b"row view" in err()               # rpi <= 0
    assert tn(yv=(0, 64, 68)) == -1 and tn(xv=(0, 64, 60)) == -1          # ld not a multiple of 8
    assert tn(yv=(100, 8, 64)) == -1 and tn(xv=(4, 8, 64)) == -1          # item stride not a multiple of 8
    assert tn(ybs=60) == -1 and b"block stride" in err()
    assert tn(xbs=4) == -1
    assert tn(M=0) == -1 and tn(N=96) == -1 and tn(K_=32) == -1 and tn(N=0) == -1 and b"multiples of 64" in err()
    assert tn(ldw=56) == -1 and b"ldw" in err()
    # a group whose contraction is split (2 jobs of 300 rows on one tile each) with a job that does not accumulate: refused by name, no launch
    assert tn(njobs=2, M=300, acc=0) == -1 and b"accumulating" in err()
    assert K.tn_group_splits((300, 300), (64, 64), (64, 64)) > 1
    assert L.mra_debug_gemm_tn_group(1, None, None, None, None, None, None, None, None, None, None, None, None, None, F16, None) == -1

    # ln_bwd ------------------------------------------------------------------------------------------------------------------------
    def job(dy=base, x=base, gamma=base, dx=base, add=None, dx16=None, dgamma=None, dbeta=None):
        return P([dy, x, gamma, dx, add, dx16, dgamma, dbeta])
    v5 = V([(0, 4, 256)] * 5)

    def lnb(pa=None, va=v5, ra=4, pb=None, vb=None, rb=0, H=256, dt=F16):
        return L.mra_debug_ln_bwd(pa if pa is not None else job(), va, ra, 1e-12, pb, vb, rb, 1e-12, H, dt, None)
    for H in (0, 128, 300, 1280, 2048):
        assert lnb(H=H) == -1 and b"H must" in err()
    assert lnb(dt=F32) == -1 and lnb(ra=-1) == -1
    assert lnb(pa=job(dy=None)) == -1 and lnb(pa=job(gamma=None)) == -1 and lnb(pa=job(dx=None)) == -1 and b"null" in err()
    assert lnb(va=V([(0, 4, 258)] + [(0, 4, 256)] * 4)) == -1 and b"multiples of 4" in err()        # dy ld
    assert lnb(va=V([(0, 4, 256), (6, 4, 256)] + [(0, 4, 256)] * 3)) == -1                           # x item stride
    assert lnb(va=V([(0, 4, 256)] * 2 + [(0, 4, 128)] + [(0, 4, 256)] * 2)) == -1 and b"below H" in err()
    assert lnb(pa=job(dx16=base), va=V([(0, 4, 256)] * 4 + [(0, 4, 260)])) == -1 and b"multiples of 8" in err()
    assert lnb(pa=job(dx16=base), va=V([(0, 4, 256)] * 4 + [(1028, 4, 256)])) == -1
    assert lnb(pa=job(add=base), va=V([(0, 4, 256)] * 3 + [(0, 0, 256), (0, 4, 256)])) == -1         # add view rpi 0
    assert lnb(pa=job(dgamma=base)) == -1 and b"pair" in err()
    assert lnb(pa=job(dbeta=base)) == -1
    assert lnb(pa=job(x=base + 4)) == -1 and b"misaligned" in err()
    assert lnb(pa=job(dgamma=base, dbeta=base), pb=job(), vb=v5, rb=4) == -1 and b"both jobs" in err()
    assert lnb(pa=job(), pb=job(dgamma=base, dbeta=base), vb=v5, rb=4) == -1
    assert lnb(rb=3) == -1 and b"without job b" in err()
    assert lnb(pb=job(x=None), vb=v5, rb=2) == -1 and b"job b" in err()
    assert lnb(ra=0) == 0 and lnb(ra=0, pb=job(), vb=v5, rb=0) == 0                                  # nothing to do: no launch

    # embed_bwd ---------------------------------------------------------------------------------------------------------------------
    def emb(demb=fake, ids=fake, items=2, Lt=4, Q=32, H=256, vocab=10, dq=fake, dp=fake, dw=fake):
        return L.mra_debug_embed_bwd(demb, ids, items, Lt, Q, H, vocab, dq, dp, dw, None)
    assert emb(H=0) == -1 and emb(H=-4) == -1 and emb(H=254) == -1 and b"H must" in err()
    assert emb(Q=-1) == -1 and emb(Lt=-1) == -1 and emb(Q=0, Lt=0) == -1 and b"Q + L" in err()
    assert emb(vocab=0) == -1 and b"vocab" in err()
    assert emb(items=-1) == -1
    assert emb(ids=None) == -1 and b"ids" in err()
    assert emb(demb=None) == -1
    assert emb(items=0) == 0

    # transpose16_batch -------------------------------------------------------------------------------------------------------------
    TRJ = L.mra_debug_transpose16_batch_scratch_bytes(1)
    assert TRJ >= 32 and L.mra_debug_transpose16_batch_scratch_bytes(3) == 3 * TRJ
    assert L.mra_debug_transpose16_batch_scratch_bytes(0) == 0 and L.mra_debug_transpose16_batch_scratch_bytes(-2) == 0

    def tr(njobs=2, src=base, dst=base, R=33, C_=7, scratch=base, nbytes=None, dt=F16):
        n = max(njobs, 1)
        return L.mra_debug_transpose16_batch(P([src] * n), P([dst] * n), I32([R] * n), I32([C_] * n), njobs, dt, scratch,
                                             n * TRJ if nbytes is None else nbytes, None)
    assert tr(njobs=0) == -1 and tr(njobs=-1) == -1 and b"njobs" in err()
    assert tr(R=0) == -1 and tr(C_=0) == -1 and tr(R=-5) == -1 and b"at least 1" in err()
    assert tr(nbytes=2 * TRJ - 1) == -1 and b"scratch" in err()
    assert tr(scratch=None) == -1 and tr(src=None) == -1 and tr(dst=None) == -1
    assert tr(dt=F32) == -1

    # gemm_gelu ---------------------------------------------------------------------------------------------------------------------
    def gg(nprob=1, A=base, W=base, Cp=base, aux=base, av=(0, 70, 192), cv=(0, 70, 128), M=70, N=128, K_=192, bwd=0, tile=_lib.GT_64, dt=F16):
        n = max(nprob, 1)
        return L.mra_debug_gemm_gelu(nprob, P([A] * n), V([av] * n), P([W] * n), None, P([Cp] * n), V([cv] * n), P([aux] * n), I32([M] * n),
                                     I32([N] * n), I32([K_] * n), bwd, tile, dt, None)
    assert gg(nprob=0) == -1 and gg(nprob=3) == -1
    assert gg(dt=F32) == -1
    assert gg(tile=4) == -1 and gg(tile=-1) == -1 and b"tile_cfg" in err()
    for bwd in (0, 1):
        assert gg(A=None, bwd=bwd) == -1 and gg(W=None, bwd=bwd) == -1 and gg(Cp=None, bwd=bwd) == -1 and gg(aux=None, bwd=bwd) == -1 and b"null" in err()
        assert gg(M=0, bwd=bwd) == -1 and gg(N=0, bwd=bwd) == -1 and gg(K_=0, bwd=bwd) == -1 and b"gemm_plan" in err()
        assert gg(K_=96, av=(0, 70, 96), bwd=bwd) == -1                                  # K % 64
        assert gg(N=96, cv=(0, 70, 96), bwd=bwd) == -1                                   # N no multiple of the 64 tile
        assert gg(tile=_lib.GT_128, N=192, cv=(0, 70, 192), bwd=bwd) == -1               # ... nor of the 128 tile
        assert gg(tile=_lib.GT_256, bwd=bwd) == -1
        assert gg(cv=(0, 70, 130), bwd=bwd) == -1 and gg(cv=(0, 0, 128), bwd=bwd) == -1  # C strides multiples of 4, rpi > 0
        assert gg(av=(0, 70, 196), bwd=bwd) == -1 and gg(av=(0, 0, 192), bwd=bwd) == -1
        assert gg(av=(0, 70, 128), bwd=bwd) == -1 and b"row stride" in err()
        assert gg(A=base + 8, bwd=bwd) == -1 and b"misaligned" in err()
