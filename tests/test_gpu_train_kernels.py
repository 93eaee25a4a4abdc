"""``-m gpu``: the kernels the Q-Former training step launches besides the attention cores, each on its own through its ``mra_debug_*``
entry (the launch functions csrc/mra_train.hip calls), against float64 references on the same rounded inputs under the DERIVED bounds of
``tests/train_kernel_cases.py`` (nothing there was fitted to this file's output; the fp32 emulations sit inside every bound and the named
mutants outside: tests/test_train_kernel_cases_cpu.py).  Every test prints its worst error / bound and asserts <= 1.

Canaries as tests/test_gpu_qformer_kernels.py: every output buffer is all-ones bits between guards of the same; after the launch exactly
the elements the kernel owns were rewritten and everything else still carries its bits -- guards, the columns between K and ldw, rows
past M, the destinations of other jobs, word rows no id hits.  Inputs sit between guards, hold NaN wherever no view addresses them, and
must come back bit for bit."""
import time

import pytest
import torch

import train_kernel_cases as K
from mraudio_amd import _lib as L
from test_gpu_qformer_kernels import DEV, DT, GUARD, Buf, _bits, _ok, _stream

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module", autouse=True)
def dev():
    assert torch.cuda.is_available()
    return torch.device(DEV)


def _ones_bits(numel, dtype):
    """CPU tensor of all-ones bits (the sentinel), to be filled in part."""
    return torch.full((numel,), -1, dtype={2: torch.int16, 4: torch.int32}[torch.empty(0, dtype=dtype).element_size()]).view(dtype)


def _nan(numel, dtype):
    return torch.full((numel,), float("nan"), dtype=dtype)


def _index(view, rows, cols, off=0):
    """Flat element indices [rows, cols] of a row view (item_stride, rows per item, row stride) from element ``off`` on."""
    m = torch.arange(rows)
    return off + ((m // view[1]) * view[0] + (m % view[1]) * view[2])[:, None] + torch.arange(cols)[None, :]


def _lay(mat, view, numel, off=0, fill=None):
    """``mat`` [rows, cols] laid out by ``view`` in a flat tensor of ``numel`` elements (NaN elsewhere unless ``fill`` is given)."""
    flat = _nan(numel, mat.dtype) if fill is None else fill
    flat[_index(view, mat.shape[0], mat.shape[1], off).reshape(-1)] = mat.reshape(-1)
    return flat


def _mask(view, rows, cols, numel, off=0):
    w = torch.zeros(numel, dtype=torch.bool)
    w[_index(view, rows, cols, off).reshape(-1)] = True
    return w


def _addr(buf, off=0):
    return buf.inner.data_ptr() + off * buf.inner.element_size()


# =========================================================================================================================================
# gemm_tn
# =========================================================================================================================================
def _tn_blocks(mat, view, block_stride, numel, off=0):
    """An operand of gemm_tn: 64-column block b of ``mat`` [M, 64 nb] starts at b * block_stride and lies by ``view``."""
    flat = _nan(numel, mat.dtype)
    for b in range(mat.shape[1] // 64):
        _lay(mat[:, 64 * b:64 * b + 64], view, numel, off + b * block_stride, fill=flat)
    return flat


def _tn_job(M, N, K_, dtype, acc=1, with_db=True, pad=8, y_layout=None, x_layout=None, seed=0):
    """One job: logical operands and their device layout.  *_layout = (view, block_stride, numel, base offset); default row-major."""
    y, x, W0, db0 = K.make_tn(M, N, K_, dtype, seed=seed)
    yl = y_layout or ((0, M, N), 64, M * N, 0)
    xl = x_layout or ((0, M, K_), 64, M * K_, 0)
    return dict(y=y, x=x, W0=W0 if acc else None, db0=db0 if with_db else None, M=M, N=N, K=K_, ldw=K_ + pad, acc=acc, yl=yl, xl=xl)


def _tn_launch(jobs, dt, expect_refusal=False):
    """Runs the jobs in ONE mra_debug_gemm_tn_group call and checks every canary.  Returns [(dW [N, K], db [N] or None)] on the CPU."""
    dtype, op = DT[dt]
    dev = []
    for j in jobs:
        N, K_, ldw = j["N"], j["K"], j["ldw"]
        yb = Buf(j["yl"][2], dtype, _tn_blocks(j["y"], j["yl"][0], j["yl"][1], j["yl"][2], j["yl"][3]))
        xb = Buf(j["xl"][2], dtype, _tn_blocks(j["x"], j["xl"][0], j["xl"][1], j["xl"][2], j["xl"][3]))
        wfill = _ones_bits(N * ldw, F32)
        if j["W0"] is not None:
            _lay(j["W0"], (0, N, ldw), N * ldw, fill=wfill)
        wb = Buf(N * ldw, F32, wfill)
        bb = Buf(N, F32, j["db0"]) if j["db0"] is not None else None
        dev.append((yb, xb, wb, bb, None if bb else Buf(N, F32, torch.zeros(N))))     # the last: a db buffer that is NOT handed over
    n = len(jobs)
    rc = L.lib().mra_debug_gemm_tn_group(
        n, K.c_ptrs([_addr(d[0], j["yl"][3]) for d, j in zip(dev, jobs)]), K.c_views([j["yl"][0] for j in jobs]), K.c_i64([j["yl"][1] for j in jobs]),
        K.c_ptrs([_addr(d[1], j["xl"][3]) for d, j in zip(dev, jobs)]), K.c_views([j["xl"][0] for j in jobs]), K.c_i64([j["xl"][1] for j in jobs]),
        K.c_ptrs([d[2] for d in dev]), K.c_ptrs([d[3] for d in dev]), K.c_i32([j["M"] for j in jobs]), K.c_i32([j["N"] for j in jobs]),
        K.c_i32([j["K"] for j in jobs]), K.c_i32([j["ldw"] for j in jobs]), K.c_i32([j["acc"] for j in jobs]), op, _stream())
    if expect_refusal:
        torch.cuda.synchronize()
        assert rc == -1, rc
        for yb, xb, wb, bb, spare in dev:
            wb.unchanged("dW of a refused group")
        return L.lib().mra_last_error()
    _ok(rc, "mra_debug_gemm_tn_group")
    out = []
    for (yb, xb, wb, bb, spare), j in zip(dev, jobs):
        yb.unchanged("dY")
        xb.unchanged("X")
        if spare:
            spare.unchanged("the db of a job without db")
        N, K_, ldw = j["N"], j["K"], j["ldw"]
        dW = wb.result(_mask((0, N, ldw), N, K_, N * ldw), "dW").view(N, ldw)[:, :K_]
        out.append((dW, bb.result(True, "db") if bb else None))
    return out


def _tn_check(jobs, outs, splits, failures, worst, what):
    for i, (j, (dW, db)) in enumerate(zip(jobs, outs)):
        rW, bW, rb, bb = K.tn_ref(j["y"], j["x"], j["W0"], j["db0"], splits)
        r = K.ratio(dW, rW, bW)
        if db is not None:
            r = max(r, K.ratio(db, rb, bb))
        worst = max(worst, (r, (what, i, j["M"], j["N"], j["K"], j["acc"])))
        if not r <= 1.0:
            failures.append((what, i, j["M"], j["N"], j["K"], j["acc"], round(r, 3)))
    return worst


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_tn_single_tile_every_tail_and_split(dt):
    """N = K = 64: one tile, splits = steps / 4.  Every residue of the 32-row tail mask (M 33 .. 64), M = 1 and 31, and the split
    contractions 257 (2 pieces), 531 (last piece 2 steps), 645 (last piece one step of 5 live rows) and 770 (last piece empty), each
    accumulating on a prefilled dW with ldw = K + 8, with db prefilled and with db NULL; 64, 257 and 770 also without accumulate (the plain
    store and the memset path: the gap columns keep the sentinel)."""
    dtype, _ = DT[dt]
    t0, worst, failures = time.time(), (0.0, None), []
    for M in K.TN_SINGLE_M:
        for with_db in (True, False):
            jobs = [_tn_job(M, 64, 64, dtype, acc=1, with_db=with_db)]
            worst = _tn_check(jobs, _tn_launch(jobs, dt), K.tn_splits(M, 64, 64), failures, worst, "acc")
    for M in (64, 257, 770):
        jobs = [_tn_job(M, 64, 64, dtype, acc=0)]
        worst = _tn_check(jobs, _tn_launch(jobs, dt), K.tn_splits(M, 64, 64), failures, worst, "store")
    print(f"gemm_tn {dt} single tile: |d| / bound {worst[0]:.3f} at {worst[1]}  [{time.time() - t0:.1f} s]")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_tn_several_tiles_and_the_layouts_of_the_training_step(dt):
    """N 128, K 192, M 100: four waves over six tiles, db from column block 0 alone.  Head-major dY as the K/V gradients lie (block = head,
    stride kv * 64, item stride heads * kv * 64, row stride 64; kv 37 and 257) against a plain X; dY as a 64-column slice of a packed
    [M, 3 N] matrix (row stride 3 N, base offset N); X as an item view (32 rows of every 41).  All accumulate."""
    dtype, _ = DT[dt]
    worst, failures = (0.0, None), []
    cases = [("tiles", _tn_job(100, 128, 192, dtype))]
    for kv in (37, 257):
        items, heads = 2, 2
        M = items * kv
        cases.append((f"head-major kv={kv}", _tn_job(M, heads * 64, 64, dtype, y_layout=((heads * kv * 64, kv, 64), kv * 64, items * heads * kv * 64, 0))))
    cases.append(("packed slice", _tn_job(70, 64, 64, dtype, y_layout=((0, 70, 192), 64, 70 * 192, 64))))
    cases.append(("item view", _tn_job(96, 64, 128, dtype, x_layout=((41 * 128, 32, 128), 64, 3 * 41 * 128, 0))))
    for what, job in cases:
        worst = _tn_check([job], _tn_launch([job], dt), K.tn_splits(job["M"], job["N"], job["K"]), failures, worst, what)
    print(f"gemm_tn {dt} tiles and layouts: |d| / bound {worst[0]:.3f} at {worst[1]}")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_gemm_tn_groups(dt):
    """2, 3 and 4 jobs of different N, K and M in one launch (grid.y covers the widest job), job 1 without db; a group of two one-tile jobs
    with 300 and 257 rows, which the launcher splits in two: every job sees every contraction row once; the same group with a job that
    does not accumulate is refused and nothing is written."""
    dtype, _ = DT[dt]
    worst, failures = (0.0, None), []
    for n in (2, 3, 4):
        jobs = [_tn_job(K.GROUP_M[i], K.GROUP_N[i], K.GROUP_K[i], dtype, with_db=(i != 1), seed=i) for i in range(n)]
        splits = K.tn_group_splits(K.GROUP_M[:n], K.GROUP_N[:n], K.GROUP_K[:n])
        worst = _tn_check(jobs, _tn_launch(jobs, dt), splits, failures, worst, f"group of {n}")
    jobs = [_tn_job(300, 64, 64, dtype, seed=5), _tn_job(257, 64, 64, dtype, seed=6)]
    splits = K.tn_group_splits((300, 257), (64, 64), (64, 64))
    assert splits == 2
    worst = _tn_check(jobs, _tn_launch(jobs, dt), splits, failures, worst, "split group")
    jobs[1] = _tn_job(257, 64, 64, dtype, acc=0, seed=6)
    assert b"accumulating" in _tn_launch(jobs, dt, expect_refusal=True)
    print(f"gemm_tn {dt} groups: |d| / bound {worst[0]:.3f} at {worst[1]}")
    assert not failures, failures


# =========================================================================================================================================
# ln_bwd
# =========================================================================================================================================
TEXT_L = 5      # the text rows of the [items, 32 + L, H] stream the views below address


def _stream_view(kind, H):
    """(view, base offset, rows per item) of the query rows or the text rows of an [items, 32 + TEXT_L, H] stream."""
    S = 32 + TEXT_L
    return ((S * H, 32, H), 0, 32) if kind == "query" else ((S * H, TEXT_L, H), 32 * H, TEXT_L)


def _lnb_job(case, rows, H, dtype, kind, add, dx16, dgrad):
    """Device buffers of one job: dy and x as the query / text rows of a stream, everything else compact.  None for an empty job."""
    if rows == 0:
        return None
    view, off, rpi = _stream_view(kind, H)
    numel = (rows + rpi - 1) // rpi * (32 + TEXT_L) * H
    j = dict(rows=rows, view=view, off=off, case=case, add=add, dgrad=dgrad)
    j["dy"] = Buf(numel, F32, _lay(case["dy"], view, numel, off))
    j["x"] = Buf(numel, F32, _lay(case["x"], view, numel, off))
    j["gamma"] = Buf(H, F32, case["gamma"])
    j["dx"] = Buf(rows * H, F32)
    j["addb"] = Buf(rows * H, F32, case["add"]) if add else None
    j["dx16"] = Buf(rows * H, dtype) if dx16 else None
    j["dg"] = Buf(H, F32, case["dgamma0"]) if dgrad else None
    j["db"] = Buf(H, F32, case["dbeta0"]) if dgrad else None
    return j


def _lnb_args(j, H):
    if j is None:
        return None, None, 0
    ptrs = K.c_ptrs([_addr(j["dy"], j["off"]), _addr(j["x"], j["off"]), j["gamma"], j["dx"], j["addb"], j["dx16"], j["dg"], j["db"]])
    plain = (0, max(j["rows"], 1), H)
    return ptrs, K.c_views([j["view"], j["view"], plain, plain, plain]), j["rows"]


def _lnb_launch(ja, jb, H, op, empty_b=False):
    """ja / jb None: an empty job.  An empty job a, or an empty job b under ``empty_b``, is handed over with 0 rows and its dgamma / dbeta
    choice alone (the two jobs must agree on it); otherwise a missing job b is a NULL job."""
    pa, va, ra = _lnb_args(ja, H)
    pb, vb, rb = _lnb_args(jb, H)
    agree = lambda j: K.c_ptrs([None] * 6 + ([j["dg"], j["db"]] if j["dgrad"] else [None, None]))   # noqa: E731
    if ja is None:
        pa = agree(jb)
    if jb is None and empty_b:
        pb = agree(ja)
    _ok(L.lib().mra_debug_ln_bwd(pa, va, ra, K.LNB_EPS, pb, vb, rb, K.LNB_EPS, H, op, _stream()), "mra_debug_ln_bwd")


def _lnb_collect(j, dtype, calls, failures, what):
    """Checks one job's buffers after ``calls`` identical launches; returns the worst ratios (dx, dgamma, dbeta)."""
    c, rows = j["case"], j["rows"]
    for name in ("dy", "x", "gamma"):
        j[name].unchanged(name)
    if j["addb"]:
        j["addb"].unchanged("add")
    H = c["gamma"].numel()
    ref = K.lnb_ref(c["x"], c["dy"], c["gamma"], K.LNB_EPS, c["add"] if j["add"] else None)
    dx = j["dx"].result(True, "dx").view(rows, H)
    r = [K.ratio(dx, ref[0], ref[1]), 0.0, 0.0]
    if j["dx16"] and not torch.equal(_bits(j["dx16"].result(True, "dx16").view(rows, H)), _bits(dx.to(dtype))):
        failures.append((what, "dx16 is not dx rounded once"))
    if j["dgrad"]:
        # `calls` identical launches are a LayerNorm backward over `calls` copies of the rows: the reference and the bound of that
        rep = K.lnb_ref(c["x"].repeat(calls, 1), c["dy"].repeat(calls, 1), c["gamma"], K.LNB_EPS, None, c["dgamma0"], c["dbeta0"])
        r[1] = K.ratio(j["dg"].result(True, "dgamma"), rep[2], rep[3])
        r[2] = K.ratio(j["db"].result(True, "dbeta"), rep[4], rep[5])
    if not max(r) <= 1.0:
        failures.append((what, [round(v, 3) for v in r]))
    return r


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("H", K.LNB_H)
def test_ln_bwd_rows_and_options(H, dt):
    """rows 1 .. 70 (wave and workgroup tails, the clamped re-read), the eight combinations of add / dx16 / dgamma+dbeta walked along the
    row counts (a different start per H), dy and x as the query rows (even positions) or the text rows (odd) of a stream, dx compact."""
    dtype, op = DT[dt]
    worst, failures, seen = [0.0, 0.0, 0.0], [], set()
    for i, rows in enumerate(K.LNB_ROWS):
        combo = (i + H // 256) % 8
        add, dx16, dgrad = bool(combo & 1), bool(combo & 2), bool(combo & 4)
        seen.add(combo)
        j = _lnb_job(K.make_lnb("normal", rows, H), rows, H, dtype, "query" if i % 2 == 0 else "text", add, dx16, dgrad)
        _lnb_launch(j, None, H, op)
        r = _lnb_collect(j, dtype, 1, failures, (rows, combo))
        worst = [max(a, b) for a, b in zip(worst, r)]
    assert len(seen) == 8
    print(f"ln_bwd {dt} H={H}: dx {worst[0]:.3f}, dgamma {worst[1]:.3f}, dbeta {worst[2]:.3f} of the bound")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("H", (768, 1024))
def test_ln_bwd_families_and_a_second_call(H, dt):
    """Rows at mean 1000, rows with one outlier of 1e4 and constant rows (xhat = 0, rstd = 1e6), 17 rows with every option on; a second
    identical launch must add the same increment to dgamma and dbeta again (held against the bound of twice the rows)."""
    dtype, op = DT[dt]
    worst, failures = {}, []
    for kind in K.LNB_FAMILIES:
        j = _lnb_job(K.make_lnb(kind, 17, H, seed=1), 17, H, dtype, "text", True, True, True)
        _lnb_launch(j, None, H, op)
        _lnb_launch(j, None, H, op)
        worst[kind] = [round(v, 3) for v in _lnb_collect(j, dtype, 2, failures, kind)]
    print(f"ln_bwd {dt} H={H} families (dx, dgamma, dbeta after two calls): {worst}")
    assert not failures, failures


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("H", (256, 768))
def test_ln_bwd_two_jobs_in_one_launch(H, dt):
    """Job a on the query rows, job b on the text rows, each with its own gamma and its own dgamma / dbeta: every job's parameter
    gradients come from its own rows alone.  (5, 0) and (0, 7) are the launcher's one-job paths."""
    dtype, op = DT[dt]
    worst, failures = [0.0, 0.0, 0.0], []
    for ra, rb in ((17, 5), (16, 1), (5, 0), (0, 7)):
        for dgrad in (True, False):
            ja = _lnb_job(K.make_lnb("normal", ra, H, seed=2), ra, H, dtype, "query", True, True, dgrad)
            jb = _lnb_job(K.make_lnb("normal", rb, H, seed=3), rb, H, dtype, "text", False, True, dgrad)
            _lnb_launch(ja, jb, H, op, empty_b=True)
            for name, j in (("a", ja), ("b", jb)):
                if j is not None:
                    r = _lnb_collect(j, dtype, 1, failures, (ra, rb, dgrad, name))
                    worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"ln_bwd {dt} H={H} two jobs: dx {worst[0]:.3f}, dgamma {worst[1]:.3f}, dbeta {worst[2]:.3f} of the bound")
    assert not failures, failures


# =========================================================================================================================================
# embed_bwd
# =========================================================================================================================================
def _emb_launch(case, c, use):
    """One launch with the outputs named in ``use`` (subset of dquery / dpos / dword) prefilled, the others NULL.  Returns the CPU tensors."""
    items, Lt, Q, H, vocab = case
    demb = Buf(c["demb"].numel(), F32, c["demb"])
    ids = Buf(max(c["ids"].numel(), 1), torch.int64, c["ids"] if Lt else torch.zeros(1, dtype=torch.int64))
    bufs = {n: (Buf(c[n + "0"].numel(), F32, c[n + "0"]) if (n in use and c[n + "0"].numel()) else None) for n in ("dquery", "dpos", "dword")}
    _ok(L.lib().mra_debug_embed_bwd(demb.ptr, ids.ptr if Lt else None, items, Lt, Q, H, vocab, bufs["dquery"].ptr if bufs["dquery"] else None,
                                    bufs["dpos"].ptr if bufs["dpos"] else None, bufs["dword"].ptr if bufs["dword"] else None, _stream()),
        "mra_debug_embed_bwd")
    demb.unchanged("demb")
    ids.unchanged("ids")
    return bufs


@pytest.mark.parametrize("case", K.EMB_CASES, ids=lambda c: "x".join(map(str, c)))
def test_embed_bwd_against_float64(case):
    """Repeated ids within and across items (at vocab 3 every row collides), ids of -1 and ``vocab``, all three outputs prefilled (+=), each
    output NULL in turn; word rows no id hits keep their prefilled bits."""
    items, Lt, Q, H, vocab = case
    c = K.make_emb(*case)
    dq, bq, dp, bp, dw, bw, hit = K.emb_ref(c["demb"], c["ids"], Q, vocab, c["dquery0"], c["dpos0"], c["dword0"])
    worst, failures = [0.0, 0.0, 0.0], []
    for use in (("dquery", "dpos", "dword"), ("dpos", "dword"), ("dquery", "dword"), ("dquery", "dpos")):
        bufs = _emb_launch(case, c, use)
        r = [0.0, 0.0, 0.0]
        if bufs["dquery"]:
            r[0] = K.ratio(bufs["dquery"].result(True, "dquery").view(Q, H), dq, bq)
        if bufs["dpos"]:
            r[1] = K.ratio(bufs["dpos"].result(True, "dpos").view(Lt, H), dp, bp)
        if bufs["dword"]:
            if Lt:
                got = bufs["dword"].result(hit[:, None].expand(vocab, H), "dword").view(vocab, H)
                r[2] = K.ratio(got, dw, bw)
            else:
                bufs["dword"].unchanged("dword without text")
        if not max(r) <= 1.0:
            failures.append((use, [round(v, 3) for v in r]))
        worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"embed_bwd {case}: dquery {worst[0]:.3f}, dpos {worst[1]:.3f}, dword {worst[2]:.3f} of the bound; {int(hit.sum())} of {vocab} word rows hit")
    assert not failures, failures


@pytest.mark.parametrize("case", [c for c in K.EMB_CASES if c[1] > 0], ids=lambda c: "x".join(map(str, c)))
def test_forward_and_backward_clamp_the_ids_alike(case):
    """The same ids through mra_debug_embed_ln: the text rows of pre32 are word[clamp(id)] + pos, and a backward whose only non-zero upstream
    row is (item n, position l) lands in the word row the forward read."""
    items, Lt, Q, H, vocab = case
    c = K.make_emb(*case)
    g = torch.Generator().manual_seed(11)
    query, word, pos = torch.randn(1, Q, H, generator=g), torch.randn(vocab, H, generator=g), torch.zeros(Lt, H)
    ids = Buf(c["ids"].numel(), torch.int64, c["ids"])
    dev = [Buf(t.numel(), F32, t) for t in (query, word, pos, torch.ones(H), torch.zeros(H))]
    h32, h16, pre = Buf(items * (Q + Lt) * H, F32), Buf(items * (Q + Lt) * H, torch.float16), Buf(items * (Q + Lt) * H, F32)
    _ok(L.lib().mra_debug_embed_ln(ids.ptr, items, Lt, Q, H, vocab, dev[0].ptr, 0, dev[1].ptr, dev[2].ptr, dev[3].ptr, dev[4].ptr, 1e-12, h32.ptr,
                                   h16.ptr, pre.ptr, L.MRA_F16, _stream()), "mra_debug_embed_ln")
    rows = pre.result(True, "pre32").view(items, Q + Lt, H)[:, Q:]
    fwd_row = torch.stack([torch.stack([(word == rows[n, l]).all(-1).nonzero()[0, 0] for l in range(Lt)]) for n in range(items)])
    assert torch.equal(fwd_row, c["ids"].clamp(0, vocab - 1))
    for n, l in {(0, min(1, Lt - 1)), (0, min(2, Lt - 1)), (items - 1, Lt - 1)}:      # the -1 and the `vocab` entries among them
        demb = torch.zeros(items, Q + Lt, H)
        demb[n, Q + l] = 1.0
        bufs = _emb_launch(case, dict(c, demb=demb, dword0=torch.zeros(vocab, H)), ("dword",))
        got = bufs["dword"].inner.cpu().view(vocab, H)
        assert got[:, 0].nonzero().view(-1).tolist() == [int(fwd_row[n, l])], (n, l, int(c["ids"][n, l]))


# =========================================================================================================================================
# transpose16_batch
# =========================================================================================================================================
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("njobs", K.TR_NJOBS)
def test_transpose16_batch_is_exact(njobs, dt):
    dtype, op = DT[dt]
    shapes = K.tr_shapes(njobs)
    srcs = [K.make_tr(R, C_, dtype, j) for j, (R, C_) in enumerate(shapes)]
    sb = [Buf(s.numel(), dtype, s) for s in srcs]
    db = [Buf(s.numel(), dtype) for s in srcs]
    nbytes = L.lib().mra_debug_transpose16_batch_scratch_bytes(njobs)
    scratch = Buf(nbytes // 8, torch.int64)
    _ok(L.lib().mra_debug_transpose16_batch(K.c_ptrs(sb), K.c_ptrs(db), K.c_i32([s[0] for s in shapes]), K.c_i32([s[1] for s in shapes]), njobs, op,
                                            scratch.ptr, nbytes, _stream()), "mra_debug_transpose16_batch")
    for j, (s, b, d) in enumerate(zip(srcs, sb, db)):
        b.unchanged(f"src {j}")
        got = d.result(True, f"dst {j}").view(s.shape[1], s.shape[0])
        assert torch.equal(_bits(got), _bits(s.T.contiguous())), f"job {j} {tuple(s.shape)}: {int((_bits(got) != _bits(s.T.contiguous())).sum())} elements differ"
    assert torch.equal(_bits(scratch.buf).cpu()[:GUARD], scratch.before[:GUARD]) and torch.equal(_bits(scratch.buf).cpu()[-GUARD:], scratch.before[-GUARD:])


# =========================================================================================================================================
# GELU epilogues
# =========================================================================================================================================
FAMILIES = range(14)
GELU_TILES = {"GT_64": (L.GT_64, L.GF_V1_64, (70, 128, 192)), "GT_128": (L.GT_128, L.GF_V1_128, (133, 256, 128)),
              "GT_256 K=192": (L.GT_256, L.GF_WS_256, (293, 512, 192)), "GT_256 K=128": (L.GT_256, L.GF_WS_256, (293, 512, 128)),
              "GT_AUTO": (L.GT_AUTO, L.GF_V1_64, (70, 256, 64))}
C_PAD, C_TAIL = 8, 3      # columns between N and the row stride of C / aux, rows past M: all keep the sentinel


def _gelu_problem(M, N, K_, dtype, item_view, with_bias, seed):
    A, W, bias, aux = K.make_gelu(M, N, K_, dtype, seed=seed, with_bias=with_bias)
    if item_view:           # rows 32 .. 40 of every item of a [M / 9, 41, K] tensor
        assert M % 9 == 0
        av, a_numel, a_off = (41 * K_, 9, K_), M // 9 * 41 * K_, 32 * K_
    else:
        av, a_numel, a_off = (0, M, K_), M * K_, 0
    return dict(A=A, W=W, bias=bias, aux=aux, M=M, N=N, K=K_, av=av, a_numel=a_numel, a_off=a_off)


def _gelu_launch(probs, backward, tile, family, dt):
    """One mra_debug_gemm_gelu call over one or two problems; asserts the family that ran.  Returns [(C [M, N], aux [M, N])]."""
    dtype, op = DT[dt]
    epi = L.EPI_GELU_BWD if backward else L.EPI_GELU_BOTH
    dev = []
    for p in probs:
        M, N, K_ = p["M"], p["N"], p["K"]
        ld, numel = N + C_PAD, (M + C_TAIL) * (N + C_PAD)
        ab = Buf(p["a_numel"], dtype, _lay(p["A"], p["av"], p["a_numel"], p["a_off"]))
        wb = Buf(N * K_, dtype, p["W"])
        bb = Buf(N, F32, p["bias"]) if (p["bias"] is not None and not backward) else None
        cb = Buf(numel, dtype)
        xb = Buf(numel, dtype, _lay(p["aux"], (0, M, ld), numel)) if backward else Buf(numel, dtype)
        dev.append((ab, wb, bb, cb, xb, ld, numel))
    before = [L.gemm_launches(f, epi) for f in FAMILIES]
    _ok(L.lib().mra_debug_gemm_gelu(len(probs), K.c_ptrs([_addr(d[0], p["a_off"]) for d, p in zip(dev, probs)]), K.c_views([p["av"] for p in probs]),
                                    K.c_ptrs([d[1] for d in dev]), K.c_ptrs([d[2] for d in dev]), K.c_ptrs([d[3] for d in dev]),
                                    K.c_views([(0, p["M"], d[5]) for d, p in zip(dev, probs)]), K.c_ptrs([d[4] for d in dev]),
                                    K.c_i32([p["M"] for p in probs]), K.c_i32([p["N"] for p in probs]), K.c_i32([p["K"] for p in probs]),
                                    int(backward), tile, op, _stream()), "mra_debug_gemm_gelu")
    ran = [L.gemm_launches(f, epi) - b for f, b in zip(FAMILIES, before)]
    assert ran == [int(f == family) for f in FAMILIES], f"families launched {ran}, expected family {family}"
    out = []
    for (ab, wb, bb, cb, xb, ld, numel), p in zip(dev, probs):
        M, N = p["M"], p["N"]
        ab.unchanged("A")
        wb.unchanged("W")
        if bb:
            bb.unchanged("bias")
        own = _mask((0, M, ld), M, N, numel)
        Cm = cb.result(own, "C").view(M + C_TAIL, ld)[:M, :N]
        if backward:
            xb.unchanged("aux")
            out.append((Cm, p["aux"]))
        else:
            out.append((Cm, xb.result(own, "aux").view(M + C_TAIL, ld)[:M, :N]))
    return out


def _gelu_check(probs, outs, backward, failures, worst, what):
    """worst: {"aux", "C", "bwd"} -> largest |d| / bound so far."""
    for i, (p, (Cm, aux)) in enumerate(zip(probs, outs)):
        if backward:
            ref, bound = K.gelu_bwd_ref(p["A"], p["W"], p["aux"])
            r = {"bwd": K.ratio(Cm, ref, bound)}
        else:
            pre, b_aux = K.gelu_both_ref(p["A"], p["W"], p["bias"])
            gref, b_c = K.gelu_of_aux_ref(aux)
            r = {"aux": K.ratio(aux, pre, b_aux), "C": K.ratio(Cm, gref, b_c)}
        for k, v in r.items():
            worst[k] = max(worst[k], v)
        if not max(r.values()) <= 1.0:
            failures.append((what, i, {k: round(v, 3) for k, v in r.items()}))


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("tile", list(GELU_TILES))
def test_gelu_epilogues_against_float64(tile, dt):
    """EPI_GELU_BOTH with and without a bias (aux within the GEMM bound of the pre-activation, C = T(gelu(aux as returned))) and EPI_GELU_BWD
    (C = T(acc gelu'(aux)), aux untouched) on one problem and -- for the three explicit tiles -- on the two-problem launch of Ctx::gemm2:
    M = (64, 27), the second problem's A the rows 32 .. 40 of every item of a [3, 41, K] tensor.  Pre-activations reach |u| = 8 through the
    bias (forward) and the aux tensor (backward).  The launch counter names the family that ran."""
    dtype, _ = DT[dt]
    cfg, family, (M, N, K_) = GELU_TILES[tile]
    worst, failures = {"aux": 0.0, "C": 0.0, "bwd": 0.0}, []
    one = lambda with_bias: [_gelu_problem(M, N, K_, dtype, False, with_bias, 0)]                                                    # noqa: E731
    two = lambda with_bias: [_gelu_problem(64, N, K_, dtype, False, with_bias, 1), _gelu_problem(27, N, K_, dtype, True, with_bias, 2)]  # noqa: E731
    for make in (one, two) if cfg != L.GT_AUTO else (one,):
        for with_bias in (True, False):
            probs = make(with_bias)
            _gelu_check(probs, _gelu_launch(probs, False, cfg, family, dt), False, failures, worst, ("both", len(probs), with_bias))
        probs = make(False)
        _gelu_check(probs, _gelu_launch(probs, True, cfg, family, dt), True, failures, worst, ("bwd", len(probs)))
    print(f"GELU epilogues {dt} {tile} (family {family}): |d| / bound aux {worst['aux']:.3f}, C of aux {worst['C']:.3f}, backward {worst['bwd']:.3f}")
    assert not failures, failures
