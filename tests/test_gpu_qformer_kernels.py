"""``-m gpu``: the hand-written kernels of the Q-Former forward, each on its own through its ``mra_debug_*`` entry (the forward's own launch
functions) or its public entry, against float64 references on the same rounded inputs under the DERIVED bounds of
``tests/qformer_kernel_cases.py`` (nothing there was fitted to this file's output; the fp32 emulations sit inside every bound and the named
mutants outside: tests/test_qformer_kernel_cases_cpu.py).  Every test prints its worst error / bound and asserts <= 1.

Canaries: every output buffer is all-ones bits (a NaN in f32, f16 and bf16) between GUARD elements of the same; after the launch every
element the kernel owns must have lost the sentinel and every other one must still carry it -- the guards, the columns between kvp and the
row stride, factor slots r >= R, rows past ``rows``.  Inputs sit between NaN guards and must come back bit for bit."""
import ctypes as C
import time

import pytest
import torch

import qformer_kernel_cases as K
from mraudio_amd import _lib as L

pytestmark = pytest.mark.gpu

GUARD = 256     # elements on either side of a buffer (a multiple of 8: 16-byte alignment survives)
DT = {"f16": (torch.float16, L.MRA_F16), "bf16": (torch.bfloat16, L.MRA_BF16)}
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def dev():
    assert torch.cuda.is_available()
    return torch.device(DEV)


def _stream():
    return L.current_stream()


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Buf:
    """``numel`` elements of ``dtype`` on the device between two guards, everything all-ones bits; ``fill`` (CPU tensor) initialises the
    inside (an input, or an in-place buffer)."""

    def __init__(self, numel, dtype, fill=None):
        self.numel = numel
        self.buf = torch.empty(numel + 2 * GUARD, dtype=dtype, device=DEV)
        _bits(self.buf).fill_(-1)
        self.inner = self.buf[GUARD:GUARD + numel]
        if fill is not None:
            self.inner.copy_(fill.reshape(-1).to(DEV))
        self.before = _bits(self.buf).cpu().clone()

    @property
    def ptr(self):
        return C.c_void_p(self.inner.data_ptr())

    def unchanged(self, what):
        assert torch.equal(_bits(self.buf).cpu(), self.before), f"{what}: an input (or its guard) was written"

    def result(self, written, what):
        """The inside as a CPU tensor after checking that exactly the elements of ``written`` (bool, numel; True = all) lost the sentinel
        bits / were rewritten and nothing else changed."""
        after = _bits(self.buf).cpu()
        w = torch.zeros(self.numel + 2 * GUARD, dtype=torch.bool)
        w[GUARD:GUARD + self.numel] = True if written is True else written.reshape(-1)
        assert torch.equal(after[~w], self.before[~w]), f"{what}: written outside its region ({int((after[~w] != self.before[~w]).sum())} elements)"
        assert (after[w] != -1).all(), f"{what}: {int((after[w] == -1).sum())} elements left unwritten"
        return self.inner.cpu()


def _ok(rc, what):
    L.check(rc, what)
    torch.cuda.synchronize()


def _view(*v):
    return (C.c_int64 * 3)(*v)


# =========================================================================================================================================
# self-attention
# =========================================================================================================================================
LSE_S = (33, 225, 257)


def _run_self_attention(q, k, v, mask, op, want_lse):
    items, heads, S, _ = q.shape
    qkv = Buf(items * S * 3 * heads * 64, q.dtype, K.pack_qkv(q, k, v))
    mk = Buf(items * S, torch.int64, mask) if mask is not None else None
    ctx = Buf(items * S * heads * 64, q.dtype)
    lse = Buf(items * heads * S, torch.float32) if want_lse else None
    _ok(L.lib().mra_debug_self_attention(qkv.ptr, mk.ptr if mk else None, op, items, S, heads, ctx.ptr, lse.ptr if lse else None, _stream()),
        "mra_debug_self_attention")
    qkv.unchanged("qkv")
    if mk:
        mk.unchanged("mask")
    out = K.unpack_ctx(ctx.result(True, "ctx").view(items, S, heads * 64), heads)
    return out, (lse.result(True, "lse").view(items, heads, S) if lse else None)


def _self_attention_sweep(items, heads, S, dt):
    dtype, op = DT[dt]
    worst, worst_lse, failures = (0.0, None), (0.0, None), []
    for kind in K.ATTN_FAMILIES:
        q, k, v = K.make_attn(kind, items, heads, S, dtype)
        for mkind in K.MASK_KINDS:
            mask = K.make_mask(mkind, items, S)
            ref, bound, lse_ref, lse_bound = K.attn_ref(q, k, v, mask)
            want_lse = S in LSE_S
            out, lse = _run_self_attention(q, k, v, mask, op, want_lse)
            r = K.worst_ratio(out, ref, bound)
            worst = max(worst, (r, (kind, mkind)))
            if not r <= 1.0:
                failures.append(("ctx", kind, mkind, round(r, 3)))
            if want_lse:
                rl = K.worst_ratio(lse, lse_ref, lse_bound)
                worst_lse = max(worst_lse, (rl, (kind, mkind)))
                if not rl <= 1.0:
                    failures.append(("lse", kind, mkind, round(rl, 3)))
                if kind in ("mild", "onehot_last"):     # the run without lse must give the same ctx bit for bit (these two families only)
                    out2, _ = _run_self_attention(q, k, v, mask, op, False)
                    if not torch.equal(_bits(out2), _bits(out)):
                        failures.append(("ctx differs without lse", kind, mkind))
    return worst, worst_lse, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("S", K.ATTN_S)
def test_self_attention_against_float64(S, dt):
    """heads 2, items 3: NULL mask, all ones, ragged, holes and an all-zero row, four score families each; from S = 225 the NULL-mask run is
    the four-wave kernel (q_rows = S > 32, K / V in place in the packed rows) and the all-ones run the masked one-wave kernel.  At S in
    LSE_S every run also writes lse; there the ``mild`` and ``onehot_last`` families (every mask kind) are run again with lse = NULL and
    must give the same ctx bit for bit -- two families, not all four: the lse store is the only difference between the runs."""
    t0 = time.time()
    worst, worst_lse, failures = _self_attention_sweep(3, 2, S, dt)
    print(f"self-attention {dt} S={S}: ctx |d| / bound {worst[0]:.3f} at {worst[1]}" +
          (f", lse |d| / bound {worst_lse[0]:.3f} at {worst_lse[1]}" if S in LSE_S else "") + f"  [{time.time() - t0:.1f} s]")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_self_attention_with_inactive_waves_in_the_last_workgroup(dt):
    """heads 1, items 3, S = 33: 6 units of one wave each, so two waves of the second workgroup are clamped to the last unit and must not
    store."""
    worst, worst_lse, failures = _self_attention_sweep(3, 1, 33, dt)
    print(f"self-attention {dt} 6 units: ctx |d| / bound {worst[0]:.3f} at {worst[1]}, lse |d| / bound {worst_lse[0]:.3f} at {worst_lse[1]}")
    assert not failures, failures


# =========================================================================================================================================
# LayerNorm family
# =========================================================================================================================================
def _params_array(sets):
    flat = []
    for s in sets:
        flat += [None, None] if s is None else [s[0].data_ptr(), s[1].data_ptr()]
    flat += [None] * (8 - len(flat))
    return (C.c_void_p * 8)(*flat)


def _dense_mask(view, rows, H, numel):
    """Elements a row view (item_stride, rpi, ld) addresses for ``rows`` rows of H columns."""
    w = torch.zeros(numel, dtype=torch.bool)
    m = torch.arange(rows)
    base = (m // view[1]) * view[0] + (m % view[1]) * view[2]
    w[(base[:, None] + torch.arange(H)[None, :]).reshape(-1)] = True
    return w


def _run_ln_rows(x_flat, xv, rows, H, sets_cpu, lane_rows, period, split, eps, op, dtype, y32v, y16v, y_numel, want32=True, want16=True):
    xb = Buf(x_flat.numel(), torch.float32, x_flat)
    sets_dev = [None if s is None else (s[0].to(DEV), s[1].to(DEV)) for s in sets_cpu]
    y32 = Buf(y_numel, torch.float32) if want32 else None
    y16 = Buf(y_numel, dtype) if want16 else None
    _ok(L.lib().mra_debug_ln_rows(xb.ptr, _view(*xv), rows, H, _params_array(sets_dev), lane_rows, period, split, eps,
                                  y32.ptr if y32 else None, _view(*y32v), y16.ptr if y16 else None, _view(*y16v), op, _stream()), "mra_debug_ln_rows")
    xb.unchanged("x")
    o32 = y32.result(_dense_mask(y32v, rows, H, y_numel), "y32") if y32 else None
    o16 = y16.result(_dense_mask(y16v, rows, H, y_numel), "y16") if y16 else None
    return o32, o16


def _check_ln(y32, y16, ref, bound, dtype, what, failures):
    r = K.worst_ratio(y32, ref, bound)
    if not r <= 1.0:
        failures.append((what, "y32", round(r, 3)))
    if y16 is not None and not torch.equal(_bits(y16), _bits(y32.to(dtype))):
        failures.append((what, "y16 is not y32 rounded once"))
    return r


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("H", K.LN_H)
def test_ln_rows_families_against_float64(H, dt):
    dtype, op = DT[dt]
    (g, b), = K.make_ln_params(1, H)
    worst, failures = (0.0, None), []
    for rows in (1, 3, 4, 5, 3 * 37):
        for kind in K.LN_FAMILIES:
            x = K.make_ln_rows(kind, rows, H)
            ref, bound = K.ln_ref(x, g.expand_as(x), b.expand_as(x), 1e-12)
            dense = (0, rows, H)
            y32, y16 = _run_ln_rows(x, dense, rows, H, [(g, b)], 0x7fffffff, 1, 1, 1e-12, op, dtype, dense, dense, rows * H)
            y32, y16 = y32.view(rows, H), y16.view(rows, H)
            worst = max(worst, (_check_ln(y32, y16, ref, bound, dtype, (kind, rows), failures), (kind, rows)))
            if kind == "constant" and not torch.equal(y32, b.expand_as(x)):
                failures.append((kind, rows, "a constant row is not the bias"))
    print(f"ln_rows {dt} H={H}: y32 |d| / bound {worst[0]:.3f} at {worst[1]}")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_ln_rows_parameter_sets_and_row_views(dt):
    """Four clearly different parameter sets (gains near 1, 2, 3, 4, biases near +10, -20, +30, -40): a wrong set on any row is gross."""
    dtype, op = DT[dt]
    H, S, N = 256, 37, 2
    sets = K.make_ln_params(4, H)
    Gs, Bs = torch.stack([s[0] for s in sets]), torch.stack([s[1] for s in sets])
    failures, worst = [], 0.0
    cases = {"two sets, period S, split 32": (N * S, [sets[0], sets[1]], 0x7fffffff, True, False),
             "four sets, lane_rows N S": (2 * N * S, sets, N * S, True, True),
             "gain4 NULL": (2 * N * S, [sets[0], sets[1], sets[2], None], N * S, True, False),
             "sets 1 and 3 only": (2 * N * S, [sets[0], None, sets[2], None], N * S, False, False)}
    for name, (rows, ss, lane_rows, have2, have4) in cases.items():
        x = K.make_ln_rows("normal", rows, H, seed=len(name))
        idx = K.ln_set_index(rows, S, 32, lane_rows, have2, have4)
        ref, bound = K.ln_ref(x, Gs[idx], Bs[idx], 1e-12)
        dense = (0, rows, H)
        y32, y16 = _run_ln_rows(x, dense, rows, H, ss, lane_rows, S, 32, 1e-12, op, dtype, dense, dense, rows * H)
        worst = max(worst, _check_ln(y32.view(rows, H), y16.view(rows, H), ref, bound, dtype, name, failures))
    # x: the 32 query rows of [S, H] items in place; y: dense rows, and rows of a wider stride (the 16 columns between rows stay untouched)
    x = K.make_ln_rows("normal", N * S, H, seed=99)
    xq = x.view(N, S, H)[:, :32].reshape(N * 32, H)
    # four sets on the viewed rows: logical rows 0 .. 31 are lane 1 (sets 1 / 2, split 20 of period 32), rows 32 .. 63 lane 2 (sets 3 / 4)
    vargs = (sets, 32, 32, 20)
    idx = K.ln_set_index(N * 32, 32, 20, 32, True, True)
    assert sorted(set(idx.tolist())) == [0, 1, 2, 3]
    ref, bound = K.ln_ref(xq, Gs[idx], Bs[idx], 1e-12)
    for name, yv, numel in (("query-row view -> dense", (0, N * 32, H), N * 32 * H), ("query-row view -> wide rows", (S * (H + 16), 32, H + 16), N * S * (H + 16))):
        y32, y16 = _run_ln_rows(x, (S * H, 32, H), N * 32, H, *vargs, 1e-12, op, dtype, yv, yv, numel)
        sel = _dense_mask(yv, N * 32, H, numel)
        worst = max(worst, _check_ln(y32[sel].view(N * 32, H), y16[sel].view(N * 32, H), ref, bound, dtype, name, failures))
        only32, _ = _run_ln_rows(x, (S * H, 32, H), N * 32, H, *vargs, 1e-12, op, dtype, yv, yv, numel, want16=False)
        _, only16 = _run_ln_rows(x, (S * H, 32, H), N * 32, H, *vargs, 1e-12, op, dtype, yv, yv, numel, want32=False)
        if not (torch.equal(_bits(only32[sel]), _bits(y32[sel])) and torch.equal(_bits(only16[sel]), _bits(y16[sel]))):
            failures.append((name, "an output changes when the other one is NULL"))
    print(f"ln_rows {dt} parameter sets and views: y32 |d| / bound {worst:.3f}")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("H", K.LN_H)
def test_embed_ln_against_float64(H, dt):
    """Every width (embed_ln_kernel<T, 1 .. 4>).  Two input modes: random embeddings with a position table (the add), and the LayerNorm
    families as query and word rows with a zero position table -- the offset rows a one-pass variance fails on, the outlier, and constant
    rows, which must come out as the bias bit for bit."""
    dtype, op = DT[dt]
    items, vocab = 3, 11
    g, b = K.make_ln_params(1, H, seed=8)[0]
    gd, bd = g.to(DEV), b.to(DEV)
    failures, worst = [], 0.0
    for Lt, per_item, fam in [(Lt, pi, fam) for Lt in (0, 1, 5) for pi in (False, True) for fam in (False, True)]:
        ids, query, word, pos = K.make_embed(items, Lt, H, vocab, per_item, families=fam)
        S = 32 + Lt
        pre = K.embed_pre(ids, query, word, pos, items, Lt).view(items * S, H)
        const = (pre == pre[:, :1]).all(-1)
        if fam:     # the families are really there: offset and constant rows among the queries, and (L = 5) among the text rows
            text = torch.arange(items * S) % S >= 32
            assert const[~text].any() and (pre[~text].mean(-1) > 900).any()
            assert Lt < 5 or (const[text].any() and (pre[text].mean(-1) > 900).any() and ((pre[text].mean(-1) - 50).abs() < 1).any())
        ref, bound = K.ln_ref(pre, g.expand_as(pre), b.expand_as(pre), 1e-12)
        idb = Buf(max(items * Lt, 1), torch.int64, ids if Lt else None)
        qb, wb, pb = Buf(query.numel(), torch.float32, query), Buf(word.numel(), torch.float32, word), Buf(pos.numel(), torch.float32, pos)
        outs = {}
        for with_pre in (True, False):
            h32, h16 = Buf(items * S * H, torch.float32), Buf(items * S * H, dtype)
            p32 = Buf(items * S * H, torch.float32) if with_pre else None
            _ok(L.lib().mra_debug_embed_ln(idb.ptr if Lt else None, items, Lt, 32, H, vocab, qb.ptr, 32 * H if per_item else 0, wb.ptr, pb.ptr,
                                           L.ptr(gd), L.ptr(bd), 1e-12, h32.ptr, h16.ptr, p32.ptr if p32 else None, op, _stream()), "mra_debug_embed_ln")
            for inp, nm in ((idb, "ids"), (qb, "query"), (wb, "word"), (pb, "pos")):
                inp.unchanged(nm)
            outs[with_pre] = (h32.result(True, "h32").view(items * S, H), h16.result(True, "h16").view(items * S, H),
                              p32.result(True, "pre32").view(items * S, H) if p32 else None)
        h32, h16, p32 = outs[True]
        what = (Lt, "per item" if per_item else "broadcast", "families" if fam else "random")
        if not torch.equal(h32[const], b.expand(int(const.sum()), H)):
            failures.append((what, "a constant row is not the bias"))
        if not torch.equal(_bits(p32), _bits(pre)):
            failures.append((what, "pre32 is not the embedding row"))
        worst = max(worst, _check_ln(h32, h16, ref, bound, dtype, what, failures))
        if not (torch.equal(_bits(outs[False][0]), _bits(h32)) and torch.equal(_bits(outs[False][1]), _bits(h16))):
            failures.append((what, "outputs change without pre32"))
    print(f"embed_ln {dt} H={H}: h32 |d| / bound {worst:.3f}")
    assert not failures, failures


X_DT = {"f32": (torch.float32, L.MRA_F32), "f16": (torch.float16, L.MRA_F16), "bf16": (torch.bfloat16, L.MRA_BF16)}


def _modality_rows(n_items, tokens, E, xdtype):
    """[n_items * tokens, E] in ``xdtype``: the LayerNorm families row by row."""
    rows = n_items * tokens
    x = torch.cat([K.make_ln_rows(K.LN_FAMILIES[r % len(K.LN_FAMILIES)], 1, E, seed=r) for r in range(rows)])
    if xdtype == torch.float16:
        x = x.clamp(-6.0e4, 6.0e4)
    return x.to(xdtype)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("E", K.MODALITY_E)
def test_modality_ln_every_bucket_against_float64(E, dt):
    """MAXC = 2 up to 1024, 3 up to 1536, 8 up to 4096: each bucket's last width, the first one past it, and rows far shorter than a wave
    (E = 8: one live lane, 63 lanes re-read the last chunk)."""
    dtype, op = DT[dt]
    n_src, tokens = 3, 5
    g, b = K.make_ln_params(1, E, seed=4)[0]
    gd, bd = g.to(DEV), b.to(DEV)
    failures, worst = [], (0.0, None)
    for xn, (xdtype, xcode) in X_DT.items():
        x = _modality_rows(n_src, tokens, E, xdtype)
        xb = Buf(x.numel(), xdtype, x)
        for index in (None, [2, 0, 2, 1]):
            items = n_src if index is None else len(index)
            src = torch.arange(n_src) if index is None else torch.tensor(index)
            xs = x.float().view(n_src, tokens, E)[src].reshape(items * tokens, E)
            ref, bound = K.ln_ref(xs, g.expand_as(xs), b.expand_as(xs), 1e-5)
            ib = Buf(items, torch.int64, src) if index is not None else None
            out = Buf(items * tokens * E, dtype)
            _ok(L.lib().mra_debug_modality_ln(xb.ptr, xcode, ib.ptr if ib else None, items, tokens, E, L.ptr(gd), L.ptr(bd), 1e-5, out.ptr, op, _stream()),
                "mra_debug_modality_ln")
            xb.unchanged("x")
            y = out.result(True, "out").view(items * tokens, E)
            r = K.worst_ratio(y, ref, K.round_bound(ref, bound, dtype))
            worst = max(worst, (r, (xn, "index" if index else "identity")))
            if not r <= 1.0:
                failures.append((xn, index, round(r, 3)))
            const = (xs == xs[:, :1]).all(-1)
            if not torch.equal(_bits(y[const]), _bits(b.to(dtype).expand(int(const.sum()), E))):
                failures.append((xn, index, "a constant row is not the bias"))
    print(f"modality_ln {dt} E={E}: out |d| / bound {worst[0]:.3f} at {worst[1]}")
    assert not failures, failures


def test_modality_ln_refuses_widths_the_kernel_cannot_take():
    x = torch.zeros(4 * 4104, device=DEV)
    out = torch.zeros(4 * 4104, dtype=torch.float16, device=DEV)
    for E in (4104, 12):
        assert L.lib().mra_debug_modality_ln(L.ptr(x), L.MRA_F32, None, 2, 2, E, L.ptr(x), L.ptr(x), 1e-5, L.ptr(out), L.MRA_F16, _stream()) == -1


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_modality_ln_through_the_public_entry(dt):
    """mra_modality_ln on a handle (enc_width a multiple of 64): the same launch, parameters from the handle."""
    dtype, op = DT[dt]
    failures = []
    for E in (512, 1408):
        cfg = L.mra_cfg()
        L.lib().mra_cfg_default(C.byref(cfg), E)
        cfg.hidden, cfg.heads, cfg.inter, cfg.layers, cfg.vocab, cfg.max_pos, cfg.llm_hidden, cfg.op_dtype = 256, 4, 256, 1, 16, 8, 0, op
        h = C.c_void_p()
        L.check(L.lib().mra_qformer_create(C.byref(cfg), C.byref(h)), "create")
        try:
            g, b = K.make_ln_params(1, E, seed=4)[0]
            for name, t in (("ln.weight", g), ("ln.bias", b)):
                td = t.to(DEV)
                L.check(L.lib().mra_qformer_load(h, name.encode(), L.ptr(td), L.MRA_F32, (C.c_int64 * 1)(E), 1, _stream()), name)
            torch.cuda.synchronize()
            x = _modality_rows(3, 5, E, torch.float32)
            xb, ib, out = Buf(x.numel(), torch.float32, x), Buf(4, torch.int64, torch.tensor([2, 0, 2, 1])), Buf(4 * 5 * E, dtype)
            _ok(L.lib().mra_modality_ln(h, xb.ptr, L.MRA_F32, ib.ptr, 4, 5, out.ptr, _stream()), "mra_modality_ln")
            xs = x.view(3, 5, E)[[2, 0, 2, 1]].reshape(20, E)
            ref, bound = K.ln_ref(xs, g.expand_as(xs), b.expand_as(xs), 1e-5)
            r = K.worst_ratio(out.result(True, "out").view(20, E), ref, K.round_bound(ref, bound, dtype))
            print(f"mra_modality_ln {dt} E={E}: out |d| / bound {r:.3f}")
            if not r <= 1.0:
                failures.append((E, round(r, 3)))
        finally:
            L.lib().mra_qformer_destroy(h)
    assert not failures, failures


# =========================================================================================================================================
# folded-attention helpers
# =========================================================================================================================================
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("kvp", K.SOFTMAX_KVP)
def test_softmax_rows_every_bucket_against_float64(kvp, dt):
    """Register buckets of 1, 2, 4, 9 and 16 float4 per thread and the three-pass kernel (kvp > 16384), each at its edge."""
    dtype, op = DT[dt]
    ld_s, ld_p = kvp + 8, kvp + 12
    failures, worst = [], (-1.0, None)
    for rows in (1, 5):
        for kv in sorted({kvp, kvp - 3, 1}):
            for kind in ("mild", "peaked"):
                s = K.make_scores(kind, rows, kv, ld_s)
                ref, bound = K.softmax_ref(s, kv, kvp, 0.125, dtype)
                sb, pb = Buf(rows * ld_s, torch.float32, s), Buf(rows * ld_p, dtype)
                _ok(L.lib().mra_debug_softmax_rows(sb.ptr, ld_s, pb.ptr, ld_p, rows, kv, kvp, 0.125, op, _stream()), "mra_debug_softmax_rows")
                sb.unchanged("S")
                written = (torch.arange(ld_p) < kvp).expand(rows, ld_p)
                p = pb.result(written, "P").view(rows, ld_p)
                r = K.worst_ratio(p[:, :kv], ref[:, :kv], bound[:, :kv])
                worst = max(worst, (r, (rows, kv, kind)))
                if not r <= 1.0:
                    failures.append((rows, kv, kind, round(r, 3)))
                if not (_bits(p[:, kv:kvp]) == 0).all():
                    failures.append((rows, kv, kind, "padding columns are not zero"))
    print(f"softmax_rows {dt} kvp={kvp}: P |d| / bound {worst[0]:.3f} at {worst[1]}")
    assert not failures, failures


TILE_COLS = 8
FACTOR_R = (32, 384, 512)


def _fold_case(ntiles, R, dtype):
    rows = 2 * R
    m, l, pt = K.make_tile_stats(rows, ntiles, TILE_COLS, dtype, seed=R)
    kvp = ntiles * TILE_COLS + 16
    ld_p = kvp + 8
    p0 = torch.empty(rows, ld_p, dtype=dtype)
    _bits(p0).fill_(-1)
    p0[:, :ntiles * TILE_COLS] = pt
    return rows, m, l, pt, kvp, ld_p, p0


@pytest.mark.parametrize("ntiles", (1, 2, 12, 64, 65))
def test_fold_rowfactor_against_float64(ntiles):
    failures, worst = [], 0.0
    for R in FACTOR_R:
        rows, m, l, pt, kvp, ld_p, p0 = _fold_case(ntiles, R, torch.float16)
        g_ref, g_bound, _ = K.factor_ref(m, l)
        mb, lb = Buf(m.numel(), torch.float32, m), Buf(l.numel(), torch.float32, l)
        got = {}
        for probe in (False, True):
            fb, pb = Buf(2 * ntiles * 512, torch.float32), Buf(rows * ld_p, torch.float16, p0)
            hist = torch.zeros(256 + 2 * GUARD, dtype=torch.int32, device=DEV)
            _ok(L.lib().mra_debug_fold_rowfactor(mb.ptr, lb.ptr, fb.ptr, rows, R, ntiles, pb.ptr, ld_p, TILE_COLS, kvp,
                                                 C.c_void_p(hist[GUARD:].data_ptr()) if probe else None, _stream()), "mra_debug_fold_rowfactor")
            mb.unchanged("stat_m"), lb.unchanged("stat_l")
            slot = (torch.arange(512) < R).expand(2, ntiles, 512)
            f = fb.result(slot, "factors").view(2, ntiles, 512)[:, :, :R].permute(0, 2, 1).reshape(rows, ntiles)
            cols = torch.arange(ld_p)
            p = pb.result(((cols >= ntiles * TILE_COLS) & (cols < kvp)).expand(rows, ld_p), "P tail").view(rows, ld_p)
            if not (torch.equal(_bits(p[:, :ntiles * TILE_COLS].contiguous()), _bits(pt.contiguous())) and (_bits(p[:, ntiles * TILE_COLS:kvp].contiguous()) == 0).all()):
                failures.append((R, probe, "P~ changed or its tail is not zero"))
            got[probe] = (f, p, hist.cpu())
        r = K.worst_ratio(got[False][0], g_ref, g_bound)
        worst = max(worst, r)
        if not r <= 1.0:
            failures.append((R, "factors", round(r, 3)))
        if not (torch.equal(_bits(got[True][0]), _bits(got[False][0])) and torch.equal(_bits(got[True][1]), _bits(got[False][1]))):
            failures.append((R, "the probe variant changes factors or P"))
        h = got[True][2]
        if not (torch.equal(h[GUARD:GUARD + 256].long(), K.hist_ref(m, l)) and (h[:GUARD] == 0).all() and (h[GUARD + 256:] == 0).all()):
            failures.append((R, "histogram"))
        if got[False][2].any():
            failures.append((R, "the plain variant touched the histogram"))
    print(f"fold_rowfactor ntiles={ntiles}: g |d| / bound {worst:.3f}")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("ntiles", (1, 2, 12, 64, 65, 128))
def test_softmax_rescale_against_float64(ntiles, dt):
    dtype, op = DT[dt]
    failures, worst = [], 0.0
    for R in FACTOR_R:
        rows, m, l, pt, kvp, ld_p, p0 = _fold_case(ntiles, R, dtype)
        g_ref, g_bound, _ = K.factor_ref(m, l)
        ref, bound = K.rescale_ref(pt, g_ref, g_bound, TILE_COLS, dtype)
        mb, lb = Buf(m.numel(), torch.float32, m), Buf(l.numel(), torch.float32, l)
        got = {}
        for probe in (False, True):
            pb = Buf(rows * ld_p, dtype, p0)
            hist = torch.zeros(256 + 2 * GUARD, dtype=torch.int32, device=DEV)
            _ok(L.lib().mra_debug_softmax_rescale(pb.ptr, ld_p, mb.ptr, lb.ptr, rows, ntiles, TILE_COLS, kvp, op,
                                                  C.c_void_p(hist[GUARD:].data_ptr()) if probe else None, _stream()), "mra_debug_softmax_rescale")
            mb.unchanged("stat_m"), lb.unchanged("stat_l")
            # (the rescaled columns may keep their bits -- a factor of 1 -- so only the zeroed tail is required to lose the sentinel)
            after = _bits(pb.buf).cpu()
            assert torch.equal(after[:GUARD], pb.before[:GUARD]) and torch.equal(after[GUARD + pb.numel:], pb.before[GUARD + pb.numel:]), "P guards written"
            p = pb.inner.cpu().view(rows, ld_p)
            if not (_bits(p[:, kvp:].contiguous()) == -1).all():
                failures.append((R, probe, "columns past kvp written"))
            if not (_bits(p[:, ntiles * TILE_COLS:kvp].contiguous()) == 0).all():
                failures.append((R, probe, "the tail is not zero"))
            got[probe] = (p, hist.cpu())
        r = K.worst_ratio(got[False][0][:, :ntiles * TILE_COLS], ref, bound)
        worst = max(worst, r)
        if not r <= 1.0:
            failures.append((R, "P", round(r, 3)))
        if not torch.equal(_bits(got[True][0].contiguous()), _bits(got[False][0].contiguous())):
            failures.append((R, "the probe variant changes P"))
        h = got[True][1]
        if not (torch.equal(h[GUARD:GUARD + 256].long(), K.hist_ref(m, l)) and (h[:GUARD] == 0).all() and (h[GUARD + 256:] == 0).all()):
            failures.append((R, "histogram"))
    print(f"softmax_rescale {dt} ntiles={ntiles}: P |d| / bound {worst:.3f}")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_transpose_pad_bit_exact(dt):
    """Both kernels: the 64 x 64 one needs C and ld_d >= 64 and multiples of 8, everything else takes the 32 x 32 one."""
    dtype, op = DT[dt]
    shapes = [(ld_d - 3, Cc, ld_d) for Cc in (40, 64, 72, 200) for ld_d in (40, 64, 72, 200)] + [(33, 200, 200), (64, 1408, 64)]
    failures = []
    g = torch.Generator().manual_seed(12)
    for R, Cc, ld_d in shapes:
        for batch in (1, 3):
            src = torch.randn(batch, R, Cc, generator=g).to(dtype)
            src_bs, dst_bs = R * Cc + 8, Cc * ld_d + 16
            s0 = torch.zeros(batch, src_bs, dtype=dtype)
            s0[:, :R * Cc] = src.view(batch, -1)
            sb, db = Buf(batch * src_bs, dtype, s0), Buf(batch * dst_bs, dtype)
            _ok(L.lib().mra_debug_transpose_pad(sb.ptr, db.ptr, R, Cc, ld_d, src_bs, dst_bs, batch, op, _stream()), "mra_debug_transpose_pad")
            sb.unchanged("src")
            d = db.result((torch.arange(dst_bs) < Cc * ld_d).expand(batch, dst_bs), "dst").view(batch, dst_bs)[:, :Cc * ld_d].view(batch, Cc, ld_d)
            if not torch.equal(_bits(d.contiguous()), _bits(K.transpose_pad_ref(src, ld_d))):
                failures.append((R, Cc, ld_d, batch))
    assert not failures, failures


# =========================================================================================================================================
# splitters
# =========================================================================================================================================
@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_splitters_bit_exact(dt):
    dtype, op = DT[dt]
    failures = []

    def run(kind, src_flat, view, rows, Cc, chunk, parts, out_numel):
        sb, db = Buf(src_flat.numel(), torch.float32, src_flat), Buf(out_numel, dtype)
        _ok(L.lib().mra_debug_split(kind, sb.ptr, _view(*view) if view else None, rows, Cc, chunk, parts, db.ptr, op, _stream()), "mra_debug_split")
        sb.unchanged("src")
        return db.result(True, "dst")

    # split_rows: (chunk 64, parts 3) and (chunk = C, parts 2), rows 1, 5 and a row view of the 32 query rows of [S, C] items
    for Cc, chunk, parts in ((256, 64, 3), (256, 256, 2), (192, 64, 2)):
        for rows in (1, 5):
            x = K.make_split_values(rows * Cc, dtype, seed=Cc + parts).view(rows, Cc)
            got = run(0, x, (0, rows, Cc), rows, Cc, chunk, parts, rows * Cc * parts).view(rows, Cc * parts)
            if not torch.equal(_bits(got), _bits(K.split_rows_ref(x, chunk, parts, dtype))):
                failures.append(("rows", Cc, chunk, parts, rows))
        S, N = 37, 2
        x = K.make_split_values(N * S * Cc, dtype, seed=5).view(N, S, Cc)
        got = run(0, x, (S * Cc, 32, Cc), N * 32, Cc, chunk, parts, N * 32 * Cc * parts).view(N * 32, Cc * parts)
        if not torch.equal(_bits(got), _bits(K.split_rows_ref(x[:, :32].reshape(N * 32, Cc), chunk, parts, dtype))):
            failures.append(("row view", Cc, chunk, parts))
    # split_weight [rows][C] -> [rows][3 C]; split_key_weight [heads * 64][E] -> [heads][E][192]
    for rows, Cc in ((3, 100), (256, 256)):
        w = K.make_split_values(rows * Cc, dtype, seed=rows).view(rows, Cc)
        got = run(1, w, None, rows, Cc, 0, 0, rows * 3 * Cc).view(rows, 3 * Cc)
        if not torch.equal(_bits(got), _bits(K.split_weight_ref(w, dtype))):
            failures.append(("weight", rows, Cc))
    for heads, E in ((1, 8), (2, 200)):
        w = K.make_split_values(heads * 64 * E, dtype, seed=E).view(heads * 64, E)
        got = run(2, w, None, heads, E, 0, 0, heads * E * 192).view(heads, E, 192)
        if not torch.equal(_bits(got), _bits(K.split_key_weight_ref(w, heads, dtype))):
            failures.append(("key weight", heads, E))
    assert not failures, failures


# =========================================================================================================================================
# scorer
# =========================================================================================================================================
def test_cosine_score_against_float64():
    items = 3
    failures, worst = [], 0.0
    for H in (4, 260, 768):
        for Q in (1, 7, 8, 9, 32):
            for t_rows in (1, items):
                z, t = K.make_cosine(items, Q, H, t_rows)
                ref, bound = K.cosine_ref(z, t)
                zb, tb = Buf(z.numel(), torch.float32, z), Buf(t.numel(), torch.float32, t)
                sim, logit = Buf(items * Q, torch.float32), Buf(items, torch.float32)
                _ok(L.lib().mra_cosine_score(zb.ptr, tb.ptr, t_rows, items, Q, H, sim.ptr, logit.ptr, _stream()), "mra_cosine_score")
                zb.unchanged("z"), tb.unchanged("t")
                s, lg = sim.result(True, "sim").view(items, Q), logit.result(True, "logit")
                r = K.worst_ratio(s, ref, bound)
                worst = max(worst, r)
                if not r <= 1.0:
                    failures.append((H, Q, t_rows, round(r, 3)))
                if not torch.equal(lg, s.amax(-1)):
                    failures.append((H, Q, t_rows, "logit is not max_q sim"))
                if s[0, 0].item() != 0.0 or (t_rows > 1 and (s[-1] != 0).any()):
                    failures.append((H, Q, t_rows, "a zero row does not score 0"))
                logit2 = Buf(items, torch.float32)
                _ok(L.lib().mra_cosine_score(zb.ptr, tb.ptr, t_rows, items, Q, H, None, logit2.ptr, _stream()), "mra_cosine_score without sim")
                if not torch.equal(logit2.result(True, "logit"), lg):
                    failures.append((H, Q, t_rows, "logit changes without sim"))
    print(f"cosine_score: sim |d| / bound {worst:.3f}")
    assert not failures, failures
