"""Shared by tests/test_qformer_kernel_cases_cpu.py and tests/test_gpu_qformer_kernels.py (not a test module): seeded inputs, float64
references, DERIVED per-element bounds and fp32 emulations (with named mutants) for the hand-written kernels of the Q-Former forward --
the masked self-attention core (csrc/attention.hip), the LayerNorm / embedding / splitter kernels (csrc/norm_embed.hip), the softmax and
transpose helpers of the folded cross-attention (csrc/fold.hip) and the cosine scorer (csrc/score.hip).  Pure torch on the CPU.

Notation: u32 = 2^-24 (unit roundoff of fp32), u = U[T] the unit roundoff of the operand type T (2^-11 f16, 2^-8 bf16).  A fp32 sum whose
longest chain of additions has ``depth`` links carries a relative error of at most depth * u32 on the sum of the magnitudes (Higham 4.4,
first order).  The row kernels add ceil(n / 64) values per lane in sequence and then cross the 64 lanes in 6 butterfly steps:
``depth(n) = ceil(n / 64) + 6`` covers every kernel below (their in-lane order is a tree of fours, shorter than the chain).

Hardware transcendentals: v_exp_f32 / v_log_f32 are specified by AMD's ISA documents to 1 ulp; the bounds take 2 u32 relative for exp2
and 2 u32 (|log2 L| + 1) absolute for log2.  That figure is taken from the ISA documentation, not measured on the kernels.

Every bound is worst-case first order, so the faithful emulations sit far below 1.0 (tests/test_qformer_kernel_cases_cpu.py prints the
ratios); no constant here was fitted to GPU output.

---- self-attention --------------------------------------------------------------------------------------------------------------------
ctx bound, the form of tests/multi_query_cases.multi_ref with kv = S:

    |ctx - ref| <= (4 u + z) (p @ |v|) + S 2^-24 max_j |v_j|

z is non-zero only on rows whose mask is all zero.  There every score is s_j sl2 - 10000 log2(e) = s_j sl2 - 14426.95 in log2 units; fp32
numbers in [8192, 16384) are 2^-10 apart, so the one rounding of that sum moves each score by at most 2^-11 log2 units (the later
subtraction of the running maximum is exact: both operands lie in one binade).  The constant's own rounding is common to all keys and
cancels.  p_j = 2^y_j / sum_i 2^y_i with every y off by at most d = 2^-11 changes by a factor within 2^(+-2 d), so
z = 2^(2 * 2^-11) - 1 = 6.8e-4 (1.39 u for f16).

lse = log2 sum_j 2^y_j with y_j = s_j sl2 + madd_j.  |d lse| <= max_j |d y_j| + (relative error of the sum) log2(e) + the log2 and the
final add.  In log2 units, over the keys a row attends:
    64 u32 sl2 max_j (|q| . |k_j|)      fp32 accumulation of the 64 products of a score (any order)
    3 u32 max_j |y_j|                   sl2 = fl(0.125 fl(log2 e)) (1 rounding), the product (1), the mask add (1; exact where madd = 0)
    256 u32                             y_j - m_new: both at most MAX_LOG2_SCORE = 128 in magnitude
    log2(e) u32 (S + 3 ceil(S / 32) + 4 + 2)   the sum of up to S probabilities in any order, three roundings per tile for the alpha
                                        rescale of l, the merge of partial sums, and exp2's 2 u32
    2 u32 (|log2 L| + 1) + u32 |lse|    v_log_f32 and the final M + log2 L; |log2 L| <= log2 S
    rows with an all-zero mask add 3 * 2^-11: the constant fl(-10000 log2 e), the score sums and M + log2 L each round at 2^-10 spacing.

---- LayerNorm family ------------------------------------------------------------------------------------------------------------------
y = d r g + b with d = x - mean, r = (var + eps)^-1/2, two-pass in fp32 over H terms, D = depth(H):
    mean         error dm <= (D + 2) u32 mean|x|            (sum, the product with fl(1 / H) or the division)
    d            the computed d_i = d_i - dm + rho_i, |rho_i| <= u32 |d_i|
    var          sum_i (d_i - dm)^2 = sum d_i^2 + H dm^2 since sum d_i = 0: relative error (2 + D + 2) u32 + dm^2 r^2
    r            half of that, + 4 u32 for sqrtf and the reciprocal
    y            three more roundings: d r, . g, + b
    |y32 - ref| <= |g| r dm + |d r g| ((10 + D / 2) u32 + dm^2 r^2 / 2) + 2 u32 |ref|
A one-pass variance E[x^2] - mean^2 has a relative error of order u32 (1 + mean^2 / var) instead: at mean 1000, var 1 that is 6 %, far
outside.  The 16-bit copy is y32 rounded once (bit for bit); where only the 16-bit row leaves (modality_ln) the bound grows by
u (|ref| + bound) + 2^-25 (the spacing of f16 subnormals; bf16 has the range of fp32).

Constant rows: the float64 answer is the bias.  fp32 agrees bit for bit only where the mean comes out exactly, so CONSTANT_ROW values are
short dyadic numbers for which fl(H c) is exact in any order and fl(fl(H c) fl(1 / H)) = c, or fl(H c) / H = c where the kernel divides (asserted on the CPU for every width used); then
d = 0 and y = bias exactly.  For other constants the bound above rightly admits |g| r dm = up to 1e6 (D + 2) u32 |c| |g| at eps = 1e-12.

---- folded-attention helpers ----------------------------------------------------------------------------------------------------------
softmax_rows  P_j = T(exp2(s_j sl2 - m) inv).  Argument error 4 u32 max|s sl2| log2 units per entry (sl2, product, m, subtraction), twice
              (entry and normaliser) times ln 2; exp2 2 u32; the sum depth(4 kvp) (a lane adds ceil(kvp / 256) values, then 6 + 3
              steps); inv and the product 2 u32:
    |P - p| <= p (u + (8 ln2 max|s sl2| + 4 + depth(4 kvp) + 3) u32) + 2^-25 [f16 subnormals] + 2^-126 [v_exp_f32 returns no fp32 subnormals]
row factors   g_t = exp2(m_t - m) / L, L = sum_t exp2(m_t - m) l_t >= 1:
    |g - ref| <= ref (16 + ln2 |m_t - m|) u32 + 2^-126          (exp2 2, the sum of <= 128 tiles depth 8 + products, inv, product; a
                                                                  factor below the smallest normal may flush to zero)
rescale       P = T(float(P~) g_t): |P - P~ g_ref| <= |P~ g_ref| (u + the factor's relative bound) + 2^-25 [f16] + 2^-126
hist          bin(min(max(256 inv, 0), 255)); the inputs keep 256 / L at least 1e-3 from an integer and inv is within 16 u32 256 = 2.5e-4
              of it, so the binning is exact.

---- scorer ----------------------------------------------------------------------------------------------------------------------------
sim = dot / (max(|z|, eps) max(|t|, eps)), D = depth(H) + 2 (the in-lane tree of four):
    |sim - ref| <= (D + 1) u32 sum|z_i t_i| / (zn tn) + |ref| (D + 6) u32
(the two norms carry half of (D + 1) u32 each, sqrt 2 x 1, product 1, division 1; rows clamped by eps have dot = 0 exactly)."""
import math

import torch

from attention_cases import LOG2E, MAX_LOG2_SCORE, U, make_qkv, worst_ratio  # noqa: F401  (re-exported for the tests)

U32 = 2.0 ** -24
HD, TILE = 64, 32
F16_SUB = 2.0 ** -25   # half the spacing of f16 subnormals


def depth(n: int) -> int:
    return (n + 63) // 64 + 6


def sub_abs(dtype) -> float:
    return F16_SUB if dtype == torch.float16 else 0.0


# =========================================================================================================================================
# self-attention
# =========================================================================================================================================
ATTN_S = (32, 33, 63, 64, 65, 160, 224, 225, 257, 544)
ATTN_FAMILIES = ("mild", "peaked", "negative", "onehot_last")
MASK_KINDS = ("null", "ones", "ragged", "holes", "zero_row")
ATTN_MUTANTS = ("mask_last_tile", "tail", "alpha", "qclamp", "lse_ln")
ZERO_ROW_REL = 2.0 ** (2 * 2.0 ** -11) - 1.0
ZERO_ROW_LSE = 3 * 2.0 ** -11
MASK_ADD = -10000.0


def make_attn(kind: str, items: int, heads: int, S: int, dtype):
    """q, k, v [items, heads, S, 64] rounded to ``dtype``: the families of attention_cases.make_qkv, one unit per (item, head)."""
    q, k, v = make_qkv(kind, items * heads, S, HD, dtype)
    return tuple(t.view(items, heads, S, HD) for t in (q, k, v))


def make_mask(kind: str, items: int, S: int):
    """[items, S] int64 or None.  ragged: valid lengths 32, a middle value and S, one per item (cyclic); holes: every text position j with
    (j - 32) % 3 == 1 or (j - 32) % 7 == 0 is zero on odd items, (j - 32) % 2 == 0 on even ones; zero_row: item 1 (or the only item) all
    zero, query columns included, the others ragged."""
    if kind == "null":
        return None
    m = torch.ones(items, S, dtype=torch.int64)
    j = torch.arange(S)
    if kind == "ones":
        return m
    lens = (32, 32 + (S - 32) // 2, S)
    if kind in ("ragged", "zero_row"):
        for i in range(items):
            m[i, lens[i % 3]:] = 0
        if kind == "zero_row":
            m[min(1, items - 1)] = 0
        return m
    if kind == "holes":
        t = j - 32
        odd = (t >= 0) & ((t % 3 == 1) | (t % 7 == 0))
        even = (t >= 0) & (t % 2 == 0)
        for i in range(items):
            m[i, odd if i % 2 else even] = 0
        return m
    raise ValueError(kind)


def attn_ref(q, k, v, mask):
    """float64 reference.  Returns (ctx [items, heads, S, 64], ctx_bound, lse [items, heads, S] in log2 units, lse_bound)."""
    u = U[q.dtype]
    items, heads, S, _ = q.shape
    qd, kd, vd = q.double(), k.double(), v.double()
    s = qd @ kd.transpose(-1, -2) / math.sqrt(HD)
    zero_row = torch.zeros(items, dtype=torch.bool)
    if mask is not None:
        s = s + ((1 - mask).double() * MASK_ADD)[:, None, None, :]
        zero_row = mask.sum(-1) == 0
    p = torch.softmax(s, -1)
    ctx = p @ vd
    A = p @ vd.abs()
    zr = zero_row.double()[:, None, None, None]
    bound = (4 * u + ZERO_ROW_REL * zr) * A + S * 2.0 ** -24 * vd.abs().amax(-2, keepdim=True)
    y = s * LOG2E                                         # log2 units, mask included
    lse = torch.logsumexp(s, -1) * LOG2E
    # the keys a row attends: everything for an unmasked or all-zero row, the mask's ones otherwise
    att = torch.ones(items, S, dtype=torch.bool) if mask is None else (mask.bool() | zero_row[:, None])
    att4 = att[:, None, None, :]
    dots = (qd.abs() @ kd.abs().transpose(-1, -2)).masked_fill(~att4, 0.0).amax(-1)
    ymax = y.abs().masked_fill(~att4, 0.0).amax(-1)
    ntiles = (S + TILE - 1) // TILE
    lse_bound = U32 * (64 * (LOG2E / 8) * dots + 3 * ymax + 256 + LOG2E * (S + 3 * ntiles + 6) + 2 * (math.log2(S) + 1) + lse.abs()) \
        + ZERO_ROW_LSE * zero_row.double()[:, None, None]
    return ctx, bound, lse, lse_bound


def attn_emulate(q, k, v, mask, mutant=None):
    """attn_kernel's arithmetic, one wave per 32-query block: 32-key tiles, fp32 scores times sl2 plus the fp32 additive mask in log2 units
    (-inf on the padding of the last tile; without a mask the padding is set to -inf), running maximum from -1e30, alpha rescale of O and l,
    P rounded to T for P V, l from the fp32 P, ctx rounded to T, lse = M + log2 L.  The four-wave kernel of long unmasked rows merges four
    such partial results in fp32: the same error terms.  Returns (ctx, lse)."""
    T = q.dtype
    items, heads, S, _ = q.shape
    f32 = torch.float32
    sl2 = torch.tensor(0.125, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    qq = q.float()
    if mutant == "qclamp":       # the row clamp min(row, q_rows - 1) taken one too low: the last row reads its neighbour's query
        qq = qq[:, :, torch.arange(S).clamp(max=max(S - 2, 0))]
    kk, vv = k.float(), v.float()
    madd = None
    if mask is not None:
        madd = ((1.0 - mask.to(f32)) * (torch.tensor(MASK_ADD, dtype=f32) * torch.tensor(LOG2E, dtype=f32)))[:, None, None, :]
    m = torch.full((items, heads, S, 1), -1e30, dtype=f32)
    l = torch.zeros_like(m)
    o = torch.zeros(items, heads, S, HD, dtype=f32)
    ninf = torch.tensor(-float("inf"))
    last_t0 = (S - 1) // TILE * TILE
    for t0 in range(0, S, TILE):
        tok = torch.arange(t0, t0 + TILE)
        src = tok.clamp(max=S - 1)
        y = (qq @ kk[:, :, src].transpose(-1, -2)) * sl2
        if madd is not None and not (mutant == "mask_last_tile" and t0 == last_t0):
            y = y + madd[..., src]
        if mutant != "tail":
            y = torch.where(tok >= S, ninf, y)
        m_new = torch.maximum(m, y.amax(-1, keepdim=True))
        alpha = torch.exp2(m - m_new) if mutant != "alpha" else torch.ones_like(m)
        p = torch.exp2(y - m_new)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p.to(T).float() @ vv[:, :, src]
        m = m_new
    lse = (m + torch.log2(l)).squeeze(-1)
    if mutant == "lse_ln":
        lse = lse * math.log(2.0)
    return (o / l).to(T), lse


def pack_qkv(q, k, v):
    """[items, heads, S, 64] x 3 -> [items, S, 3 * heads * 64] (q | k | v thirds, heads side by side)."""
    n, h, S, d = q.shape
    return torch.cat([t.transpose(1, 2).reshape(n, S, h * d) for t in (q, k, v)], dim=-1).contiguous()


def unpack_ctx(ctx, heads: int):
    """[items, S, heads * 64] -> [items, heads, S, 64]."""
    n, S, w = ctx.shape
    return ctx.view(n, S, heads, w // heads).transpose(1, 2)


# =========================================================================================================================================
# LayerNorm family
# =========================================================================================================================================
LN_H = (256, 512, 768, 1024)
LN_FAMILIES = ("normal", "offset1000", "offset50_small", "constant", "outlier")
LN_MUTANTS = ("one_pass", "wrong_set")
CONSTANT_ROW = (1.5, -2.5, 0.75, 3.0)   # short dyadic values (module docstring); row r of a constant input holds CONSTANT_ROW[r % 4]
MODALITY_E = (8, 504, 512, 1024, 1032, 1408, 1536, 1544, 4096)


def make_ln_rows(kind: str, rows: int, H: int, seed: int = 0):
    """fp32 [rows, H]."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + rows + sum(map(ord, kind)))
    x = torch.randn(rows, H, generator=g)
    if kind == "normal":
        return x
    if kind == "offset1000":
        return 1000.0 + x
    if kind == "offset50_small":
        return x * 1e-3 + 50.0
    if kind == "constant":
        c = torch.tensor(CONSTANT_ROW)[torch.arange(rows) % len(CONSTANT_ROW)]
        return c[:, None].expand(rows, H).contiguous()
    if kind == "outlier":
        x[torch.arange(rows), (torch.arange(rows) * 37 + 5) % H] = 1.0e4
        return x
    raise ValueError(kind)


def make_ln_params(nsets: int, H: int, seed: int = 3):
    """``nsets`` clearly different (gain, bias) pairs, fp32 [H]: set s has gain around s + 1 and bias around 10 (s + 1)."""
    g = torch.Generator().manual_seed(seed + H)
    return [((s + 1.0) + 0.1 * torch.randn(H, generator=g), 10.0 * (s + 1) * (1 if s % 2 == 0 else -1) + torch.randn(H, generator=g)) for s in range(nsets)]


def ln_set_index(rows: int, period: int, split: int, lane_rows: int, have2: bool, have4: bool):
    """Parameter set (0-based) of every row as launch_ln_rows4 documents it."""
    r = torch.arange(rows)
    lane = (r >= lane_rows).long()
    second = (r % period >= split)
    second = torch.where(lane.bool(), second & have4, second & have2)
    return lane * 2 + second.long()


def ln_ref(x, gain, bias, eps: float):
    """x [rows, H] fp32, gain / bias [rows, H] (already selected per row) -> (y float64, bound)."""
    H = x.shape[-1]
    D = depth(H)
    xd, g, b = x.double(), gain.double(), bias.double()
    mean = xd.mean(-1, keepdim=True)
    d = xd - mean
    var = (d * d).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    y = d * r * g + b
    dm = (D + 2) * U32 * xd.abs().mean(-1, keepdim=True)
    bound = g.abs() * r * dm + (d * r * g).abs() * ((10 + D / 2) * U32 + 0.5 * (dm * r) ** 2) + 2 * U32 * y.abs()
    return y, bound


def ln_emulate(x, gain, bias, eps: float, mutant=None, by_division=False):
    """Two-pass fp32 LayerNorm as the kernels compute it (torch's fp32 sums stand in for the wave reduction).  ``one_pass``: variance as
    E[x^2] - mean^2."""
    H = x.shape[-1]
    f32 = torch.float32
    inv_h = torch.tensor(1.0 / H, dtype=f32)
    s = x.sum(-1, keepdim=True)
    mean = s / H if by_division else s * inv_h
    if mutant == "one_pass":
        q = (x * x).sum(-1, keepdim=True)
        var = (q / H if by_division else q * inv_h) - mean * mean
        d = x - mean
    else:
        d = x - mean
        q = (d * d).sum(-1, keepdim=True)
        var = q / H if by_division else q * inv_h
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=f32))
    return d * rstd * gain + bias


def constant_rows_are_exact(H: int, by_division: bool) -> bool:
    """fl(H c) is exact and fl(H c) / H == c (modality_ln divides) or fl(fl(H c) fl(1 / H)) == c (ln_rows / embed_ln multiply) for every
    CONSTANT_ROW value: the fp32 mean of a constant row is the constant."""
    c = torch.tensor(CONSTANT_ROW, dtype=torch.float32)
    tot = c * H
    exact_sum = torch.equal(tot.double(), c.double() * H)
    mean = tot / H if by_division else tot * torch.tensor(1.0 / H, dtype=torch.float32)
    return exact_sum and torch.equal(mean, c)


def round_bound(ref, bound, dtype):
    """Bound of a value that leaves only as T: the fp32 bound, the rounding to T and the f16 subnormal spacing."""
    return bound + U[dtype] * (ref.abs() + bound) + sub_abs(dtype)


def mixed_rows(rows: int, H: int, seed: int = 0):
    """fp32 [rows, H]: row r from LN_FAMILIES[r % 5] (a constant row holds CONSTANT_ROW[0])."""
    return torch.cat([make_ln_rows(LN_FAMILIES[r % len(LN_FAMILIES)], 1, H, seed=seed + r) for r in range(rows)])


def make_embed(items: int, L: int, H: int, vocab: int, per_item_query: bool, seed: int = 5, families: bool = False):
    """ids [items, L] with 0, vocab - 1, a negative and an id >= vocab among them; query [1 or items, 32, H], word [vocab, H], pos [max(L, 1), H].
    ``families``: the query rows and the word rows are the LayerNorm families row by row (mixed_rows) and pos is zero, so the offset,
    constant and outlier rows reach the kernel's LayerNorm unchanged; otherwise N(0, 1) queries, word ~ 0.25 + 0.5 N, pos ~ 0.5 N (the
    position add is exercised)."""
    g = torch.Generator().manual_seed(seed * 100 + L * 10 + H + items)
    ids = torch.randint(0, vocab, (items, L), generator=g)
    special = (0, vocab - 1, -3, vocab + 5, vocab)
    flat = ids.view(-1)
    for i in range(flat.numel()):
        if i < len(special) or i % 4 == 3:
            flat[i] = special[i % len(special)]
    nq = items if per_item_query else 1
    if families:
        query = mixed_rows(nq * 32, H, seed=seed).view(nq, 32, H)
        word = mixed_rows(vocab, H, seed=seed + 500)
        pos = torch.zeros(max(L, 1), H)
        if L >= 5:      # ids 1, 2, 3: an offset1000, an offset50_small and a constant word row, whatever the draw
            ids[-1, -3:] = torch.tensor([1, 2, 3])
    else:
        query = torch.randn(nq, 32, H, generator=g)
        word = torch.randn(vocab, H, generator=g) * 0.5 + 0.25
        pos = torch.randn(max(L, 1), H, generator=g) * 0.5
    return ids, query, word, pos


def embed_pre(ids, query, word, pos, items: int, L: int):
    """The rows before the LayerNorm, fp32 [items, 32 + L, H]: the query rows as they are, word[clamp(id)] + pos (one fp32 rounding)."""
    vocab = word.shape[0]
    q = query.expand(items, -1, -1) if query.shape[0] == 1 else query
    if L == 0:
        return q.contiguous()
    text = word[ids.clamp(0, vocab - 1)] + pos[None, :L]
    return torch.cat([q, text], dim=1).contiguous()


# =========================================================================================================================================
# folded-attention helpers
# =========================================================================================================================================
SOFTMAX_KVP = (4, 1024, 1028, 2048, 4096, 4100, 9216, 16384, 16388)
SOFTMAX_MUTANTS = ("tail_counted",)
FACTOR_MUTANTS = ("first_tile_max",)
TAIL_FILL = 30.0   # what the padding columns kv .. ld_s - 1 of the score rows hold: larger than any score, so a kernel that reads them shows


def make_scores(kind: str, rows: int, kv: int, ld_s: int, seed: int = 0):
    """fp32 [rows, ld_s]: scores in columns [0, kv), TAIL_FILL beyond.  scale = 0.125; mild |s sl2| ~ 1.4, peaked up to ~ 70."""
    g = torch.Generator().manual_seed(seed * 31 + kv * 7 + rows + (0 if kind == "mild" else 1))
    s = torch.full((rows, ld_s), TAIL_FILL)
    s[:, :kv] = torch.randn(rows, kv, generator=g) * (8.0 if kind == "mild" else 80.0)
    assert s[:, :kv].abs().max().item() * 0.125 * LOG2E <= MAX_LOG2_SCORE
    return s


def softmax_ref(s, kv: int, kvp: int, scale: float, dtype):
    """(P float64 [rows, kvp] with zero columns from kv on, bound)."""
    sd = s[:, :kv].double() * scale
    p = torch.softmax(sd, -1)
    amax = (sd * LOG2E).abs().amax(-1, keepdim=True)
    rel = U[dtype] + (8 * math.log(2.0) * amax + 4 + depth(4 * kvp) + 3) * U32
    out = torch.zeros(s.shape[0], kvp, dtype=torch.float64)
    bound = torch.zeros_like(out)
    out[:, :kv] = p
    bound[:, :kv] = p * rel + sub_abs(dtype) + 2.0 ** -126
    return out, bound


def softmax_emulate(s, kv: int, kvp: int, scale: float, dtype, mutant=None):
    f32 = torch.float32
    sl2 = torch.tensor(scale, dtype=f32) * torch.tensor(LOG2E, dtype=f32)
    n = kvp if mutant == "tail_counted" else kv
    x = s[:, :n]
    m = x.amax(-1, keepdim=True) * sl2
    e = torch.exp2(x * sl2 - m)
    inv = 1.0 / e.sum(-1, keepdim=True)
    out = torch.zeros(s.shape[0], kvp, dtype=dtype)
    out[:, :n] = (e * inv).to(dtype)
    return out


def make_tile_stats(rows: int, ntiles: int, tile_cols: int, dtype, seed: int = 0):
    """A float64 score row (log2 units) per row, split into ``ntiles`` tiles the way the scores GEMM's epilogue leaves it:
    stat_m [rows, ntiles] fp32 tile maxima, stat_l fp32 tile sums of exp2(s - m_tile), ptilde [rows, ntiles * tile_cols] in T.  One tile of
    every row (tile r % ntiles, unless it holds the row maximum) sits 200 below the rest: its factor underflows.  Rows are re-drawn until
    256 / L is at least 1e-3 from an integer (hist_is_safe)."""
    g = torch.Generator().manual_seed(seed * 17 + rows * 3 + ntiles * 5 + tile_cols)

    def draw(n, sharp):
        x = torch.randn(n, ntiles, tile_cols, generator=g, dtype=torch.float64) * 3.0
        x[sharp] *= 4.0
        if ntiles > 1:
            r = torch.arange(n)
            low = r % ntiles
            low = torch.where(low == x.amax(-1).argmax(-1), (low + 1) % ntiles, low)
            x[r, low] -= 200.0
        return x

    s = draw(rows, torch.arange(rows) % 3 == 0)          # every third row is peaked: its softmax maximum lands in a high bin
    for _ in range(64):
        m32 = s.amax(-1).float()
        l32 = torch.exp2(s - m32.double()[..., None]).sum(-1).float()
        bad = ~hist_is_safe(m32, l32)
        if not bad.any():
            break
        s[bad] = draw(int(bad.sum()), torch.zeros(int(bad.sum()), dtype=torch.bool))
    assert not bad.any()
    pt = torch.exp2(s - m32.double()[..., None]).to(dtype).reshape(rows, ntiles * tile_cols)
    return m32, l32, pt


def factor_ref(stat_m, stat_l):
    """(factors float64 [rows, ntiles], bound, inv = 1 / L float64 [rows])."""
    m, l = stat_m.double(), stat_l.double()
    mr = m.amax(-1, keepdim=True)
    w = torch.exp2(m - mr)
    L = (w * l).sum(-1, keepdim=True)
    g = w / L
    bound = g * (16 + math.log(2.0) * (m - mr).abs()) * U32 + 2.0 ** -126
    return g, bound, (1.0 / L).squeeze(-1)


def hist_is_safe(stat_m, stat_l):
    """[rows] bool: 256 / L at least 1e-3 from an integer, so the fp32 bin equals the float64 bin."""
    _, _, inv = factor_ref(stat_m, stat_l)
    x = inv * 256.0
    return (x - x.round()).abs() >= 1e-3


def hist_ref(stat_m, stat_l):
    _, _, inv = factor_ref(stat_m, stat_l)
    bins = (inv * 256.0).clamp(0.0, 255.0).floor().long()
    return torch.bincount(bins, minlength=256)


def factor_emulate(stat_m, stat_l, mutant=None):
    m = stat_m[:, :1] if mutant == "first_tile_max" else stat_m.amax(-1, keepdim=True)
    w = torch.exp2(stat_m - m)
    inv = 1.0 / (w * stat_l).sum(-1, keepdim=True)
    return w * inv


def rescale_ref(ptilde, g_ref, g_bound, tile_cols: int, dtype):
    """P after the rescale pass: float64 [rows, ntiles * tile_cols] and its bound."""
    g = g_ref.repeat_interleave(tile_cols, -1)
    gb = g_bound.repeat_interleave(tile_cols, -1)
    ref = ptilde.double() * g
    bound = ref.abs() * U[dtype] + ptilde.double().abs() * gb * (1 + U[dtype]) + sub_abs(dtype) + 2.0 ** -126
    return ref, bound


def transpose_pad_ref(src, ld_d: int):
    """src [batch, R, C] -> [batch, C, ld_d] with zero columns from R on."""
    b, R, C = src.shape
    out = torch.zeros(b, C, ld_d, dtype=src.dtype)
    out[:, :, :R] = src.transpose(1, 2)
    return out


# =========================================================================================================================================
# splitters
# =========================================================================================================================================
def make_split_values(n: int, dtype, seed: int = 0):
    """fp32 [n]: N(0, 1), zeros of both signs, tiny values whose lo is subnormal in f16 or underflows, magnitudes up to the f16 maximum."""
    g = torch.Generator().manual_seed(seed + n)
    x = torch.randn(n, generator=g)
    special = torch.tensor([0.0, -0.0, 65504.0, -65504.0, 60000.3, 1.0, 1.0 + 2.0 ** -12, 2.0 ** -14, 2.0 ** -14 * 1.0003, 3.1e-5, 6.1e-5, 1e-7, -1e-7,
                            2.0 ** -24, 2.0 ** -25, 5.9e-8, 1e-10, 1e-30, 1e-36, 1234.567, -0.1, 33000.7])
    k = min(n, special.numel())
    x[:k] = special[:k]
    scale = torch.tensor([1.0, 1e-3, 1e-5, 300.0])[torch.arange(n) % 4]
    x[k:] = x[k:] * scale[k:]
    return x


def split_ref(x, dtype):
    hi = x.to(dtype)
    lo = (x - hi.float()).to(dtype)
    return hi, lo


def split_rows_ref(x, chunk: int, parts: int, dtype):
    """x [rows, C] -> [rows, C / chunk, parts, chunk] flattened per row: (hi, lo, hi) or (hi, lo)."""
    rows, Cc = x.shape
    hi, lo = split_ref(x, dtype)
    hi, lo = hi.view(rows, Cc // chunk, 1, chunk), lo.view(rows, Cc // chunk, 1, chunk)
    return torch.cat([hi, lo, hi][:parts], dim=2).reshape(rows, Cc * parts)


def split_weight_ref(w, dtype):
    hi, lo = split_ref(w, dtype)
    return torch.cat([hi, hi, lo], dim=1)


def split_key_weight_ref(w, heads: int, dtype):
    """w [heads * 64, E] -> [heads, E, 192] = (hi | hi | lo) over the 64 head dimensions."""
    E = w.shape[1]
    hi, lo = split_ref(w, dtype)
    hi, lo = hi.view(heads, 64, E).transpose(1, 2), lo.view(heads, 64, E).transpose(1, 2)
    return torch.cat([hi, hi, lo], dim=2).contiguous()


# =========================================================================================================================================
# scorer
# =========================================================================================================================================
COS_EPS = 1e-8


def make_cosine(items: int, Q: int, H: int, t_rows: int, seed: int = 0):
    """z [items, Q, H], t [t_rows, H] fp32.  Edge rows: z[0, 0] = 0, (Q > 1) z[0, 1] antiparallel and (Q > 2) z[0, -1] parallel to its t
    row; with t_rows == items > 1 the last t row is zero."""
    g = torch.Generator().manual_seed(seed + items * 1000 + Q * 37 + H)
    z = torch.randn(items, Q, H, generator=g)
    t = torch.randn(t_rows, H, generator=g)
    if t_rows > 1:
        t[-1] = 0.0
    if Q > 2:
        z[0, -1] = 2.5 * t[0]
    if Q > 1:
        z[0, 1] = -0.5 * t[0]
    z[0, 0] = 0.0
    return z, t


def cosine_ref(z, t):
    items, Q, H = z.shape
    D = depth(H) + 2
    zd, td = z.double(), (t.double() if t.shape[0] > 1 else t.double().expand(items, -1))
    dot = (zd * td[:, None]).sum(-1)
    ab = (zd.abs() * td.abs()[:, None]).sum(-1)
    zn = zd.norm(dim=-1).clamp_min(COS_EPS)
    tn = td.norm(dim=-1).clamp_min(COS_EPS)[:, None]
    sim = dot / (zn * tn)
    bound = (D + 1) * U32 * ab / (zn * tn) + sim.abs() * (D + 6) * U32 + 1e-38
    return sim, bound


def cosine_emulate(z, t):
    items = z.shape[0]
    tt = t if t.shape[0] > 1 else t.expand(items, -1)
    dot = (z * tt[:, None]).sum(-1)
    zn = z.pow(2).sum(-1).sqrt().clamp_min(COS_EPS)
    tn = tt.pow(2).sum(-1).sqrt().clamp_min(COS_EPS)[:, None]
    return dot / (zn * tn)
