// C ABI (include/mra.h) and the host-side orchestration of the Q-Former forward, with the scorer's entries and the per-kernel debug
// entries behind it.  The training path is mra_train.hip, the attached LM's entries (mra_lora_*, mra_lm_head_ce_*, mra_decode_attention,
// mra_prefill_attention, mra_lm_step, mra_gather_rows) are mra_lm.hip, the encoders and front ends have their own units.
//
// Mirrors, launch by launch, what the reference gets from LAVIS' BertModel when it calls
// {modality}_Qformer.bert(...) at models/xinstructblip.py:286-293 (layer structure as stated by
// the HF port, modeling_instructblip.py:591-709), re-planned for gfx950:
//   * the K/V projections of all cross-attention layers read the same encoder features, so they
//     run as ONE GEMM [items*kv, E] x [n_cross*2*H, E]^T whose epilogue scatters into a head-major
//     K/V cache ([kv][64] contiguous per (layer, k|v, item, head)) -- the layout the attention
//     kernel streams with full 128-byte rows;
//   * query rows and text rows of the [items, 32+L, H] residual stream are addressed in place
//     through row views (no slicing copies); the two feed-forwards run as one grouped launch;
//   * residual stream, LayerNorm statistics and softmax are fp32; only MFMA operands are f16/bf16.
// No allocation and no synchronisation after create/load; everything is enqueued on `stream`.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "mra_handle.h"

using namespace mra;
using namespace mra_host;

namespace mra_host {
thread_local std::string g_err;
}

namespace {

// Lays the parameter arena out; with base == nullptr only measures.
size_t layout_params(mra_qformer* h, char* base) {
  const mra_cfg& c = h->cfg;
  const size_t H = c.hidden, I = c.inter, E = c.enc_width;
  Carver cv(base);
  size_t goff = 0;
  auto reg = [&](const std::string& name, void* p, int dtype, long long numel) {
    Param pr;
    pr.ptr = p;
    pr.dtype = dtype;
    pr.numel = numel;
    pr.goff = goff;  // gradients: one f32 block per parameter, registration order
    goff += align_up((size_t)numel * 4);
    h->params[name] = pr;
  };
  const int opd = c.op_dtype;
  h->params.clear();
  h->layers.assign(c.layers, LayerW{});
  h->word = cv.take<float>((size_t)c.vocab * H);
  h->pos = cv.take<float>((size_t)c.max_pos * H);
  h->embg = cv.take<float>(H);
  h->embb = cv.take<float>(H);
  h->query = cv.take<float>((size_t)c.n_query * H);
  h->encg = cv.take<float>(E);
  h->encb = cv.take<float>(E);
  reg("bert.embeddings.word_embeddings.weight", h->word, MRA_F32, (long long)c.vocab * H);
  reg("bert.embeddings.position_embeddings.weight", h->pos, MRA_F32, (long long)c.max_pos * H);
  reg("bert.embeddings.LayerNorm.weight", h->embg, MRA_F32, H);
  reg("bert.embeddings.LayerNorm.bias", h->embb, MRA_F32, H);
  reg("query_tokens", h->query, MRA_F32, (long long)c.n_query * H);
  reg("ln.weight", h->encg, MRA_F32, E);
  reg("ln.bias", h->encb, MRA_F32, E);
  h->ncross = 0;
  for (int i = 0; i < c.layers; ++i)
    if (i % c.cross_freq == 0) ++h->ncross;
  h->wkv = cv.take<char>((size_t)h->ncross * 2 * H * E, 2);
  h->bkv = cv.take<float>((size_t)h->ncross * 2 * H);
  h->wk32 = cv.take<float>((size_t)h->ncross * H * E);
  if (c.llm_hidden > 0) {
    h->wllm = cv.take<char>((size_t)c.llm_hidden * H, 2);
    h->bllm = cv.take<float>(c.llm_hidden);
    reg("llm_proj.weight", h->wllm, opd, (long long)c.llm_hidden * H);
    reg("llm_proj.bias", h->bllm, MRA_F32, c.llm_hidden);
  }
  int cl = 0;
  for (int i = 0; i < c.layers; ++i) {
    LayerW& L = h->layers[i];
    const std::string p = "bert.encoder.layer." + std::to_string(i) + ".";
    char* wqkv = cv.take<char>(3 * H * H, 2);
    L.wqkv = wqkv;
    L.bqkv = cv.take<float>(3 * H);
    const char* names[3] = {"query", "key", "value"};
    for (int j = 0; j < 3; ++j) {
      reg(p + "attention.self." + names[j] + ".weight", wqkv ? wqkv + (size_t)j * H * H * 2 : nullptr, opd, H * H);
      reg(p + "attention.self." + names[j] + ".bias", L.bqkv ? L.bqkv + j * H : nullptr, MRA_F32, H);
    }
    L.wo = cv.take<char>(H * H, 2);
    L.bo = cv.take<float>(H);
    L.ln1g = cv.take<float>(H);
    L.ln1b = cv.take<float>(H);
    reg(p + "attention.output.dense.weight", L.wo, opd, H * H);
    reg(p + "attention.output.dense.bias", L.bo, MRA_F32, H);
    reg(p + "attention.output.LayerNorm.weight", L.ln1g, MRA_F32, H);
    reg(p + "attention.output.LayerNorm.bias", L.ln1b, MRA_F32, H);
    L.cross_index = -1;
    if (i % c.cross_freq == 0) {
      L.cross_index = cl;
      L.wcq = cv.take<char>(H * H, 2);
      L.wcq32 = cv.take<float>(H * H);
      L.bcq = cv.take<float>(H);
      L.wco = cv.take<char>(H * H, 2);
      L.bco = cv.take<float>(H);
      L.lncg = cv.take<float>(H);
      L.lncb = cv.take<float>(H);
      reg(p + "crossattention.self.query.weight", L.wcq, opd, H * H);
      h->params[p + "crossattention.self.query.weight"].copy32 = L.wcq32;
      reg(p + "crossattention.self.query.bias", L.bcq, MRA_F32, H);
      char* wkv = (char*)h->wkv;
      reg(p + "crossattention.self.key.weight", wkv ? wkv + (size_t)(cl * 2 + 0) * H * E * 2 : nullptr, opd, H * E);
      h->params[p + "crossattention.self.key.weight"].copy32 = h->wk32 ? h->wk32 + (size_t)cl * H * E : nullptr;
      reg(p + "crossattention.self.key.bias", h->bkv ? h->bkv + (size_t)(cl * 2 + 0) * H : nullptr, MRA_F32, H);
      reg(p + "crossattention.self.value.weight", wkv ? wkv + (size_t)(cl * 2 + 1) * H * E * 2 : nullptr, opd, H * E);
      reg(p + "crossattention.self.value.bias", h->bkv ? h->bkv + (size_t)(cl * 2 + 1) * H : nullptr, MRA_F32, H);
      reg(p + "crossattention.output.dense.weight", L.wco, opd, H * H);
      reg(p + "crossattention.output.dense.bias", L.bco, MRA_F32, H);
      reg(p + "crossattention.output.LayerNorm.weight", L.lncg, MRA_F32, H);
      reg(p + "crossattention.output.LayerNorm.bias", L.lncb, MRA_F32, H);
      ++cl;
    }
    L.wit = cv.take<char>(I * H, 2);
    L.bit = cv.take<float>(I);
    L.wot = cv.take<char>(H * I, 2);
    L.bot = cv.take<float>(H);
    L.lntg = cv.take<float>(H);
    L.lntb = cv.take<float>(H);
    L.wiq = cv.take<char>(I * H, 2);
    L.biq = cv.take<float>(I);
    L.woq = cv.take<char>(H * I, 2);
    L.boq = cv.take<float>(H);
    L.lnqg = cv.take<float>(H);
    L.lnqb = cv.take<float>(H);
    reg(p + "intermediate.dense.weight", L.wit, opd, I * H);
    reg(p + "intermediate.dense.bias", L.bit, MRA_F32, I);
    reg(p + "output.dense.weight", L.wot, opd, H * I);
    reg(p + "output.dense.bias", L.bot, MRA_F32, H);
    reg(p + "output.LayerNorm.weight", L.lntg, MRA_F32, H);
    reg(p + "output.LayerNorm.bias", L.lntb, MRA_F32, H);
    reg(p + "intermediate_query.dense.weight", L.wiq, opd, I * H);
    reg(p + "intermediate_query.dense.bias", L.biq, MRA_F32, I);
    reg(p + "output_query.dense.weight", L.woq, opd, H * I);
    reg(p + "output_query.dense.bias", L.boq, MRA_F32, H);
    reg(p + "output_query.LayerNorm.weight", L.lnqg, MRA_F32, H);
    reg(p + "output_query.LayerNorm.bias", L.lnqb, MRA_F32, H);
  }
  h->grad_bytes = goff;
  return cv.off;
}

// How a forward runs its cross-attention layers: the one place that turns the handle's cross mode, with the precision and the probe the
// caller asks for, into a form, its buffers (layout_cross) and its launches (cross_core).
struct CrossPlan {
  enum Form { KV_CACHE, FOLD, FOLD_STREAM } form;
  bool precise;    // split precision: hi + lo pairs along the score chain (folded form)
  bool probe;      // the probing forward of the automatic precision: the row-factor / rescale kernels write the p_max histograms
  // the folded form on the batched GEMMs (FOLD):
  bool kmajor;     // P . enc reads the encoder tokens themselves (K-major weights): no enc^T copy
  bool softpart;   // scores on the 176 x 384 EPI_SOFTPART tile (otherwise fp32 scores + a row softmax)
  bool inreg;      // with softpart: P . enc applies the row factors to its P~ fragments (otherwise a rescale pass over P)
  bool raw;        // the encoder features are RAW (no modality LayerNorm pass): its gain and centring live in the folded weights, the token
                   // factors 1 / sqrt(var + eps) come out of cross layer 0's scores launch (FOLD with softpart && kmajor && inreg only)
  bool fuse_query; // steps 5 + 6a in one launch (launch_fold_query): the default folded plan with "cross_fuse" bit 1, 64-wide heads
  bool stat_factors; // step 6c inside the P . enc launch (GemmProb::ps_stats): no fold_rowfactor launch, no factor array ("cross_fuse" bit 2)
  bool ctx_64;     // step 6e on the 64 x 64 tile with 128-deep K steps ("cross_fuse" bit 4): twice the workgroups, each pulls 2/3 of the bytes
  int scores_tile, penc_tile;   // GemmTile of the scores and the P . enc GEMMs
};

CrossPlan cross_plan(const mra_qformer* h, int kv, bool precise, bool probe, bool raw = false) {
  const mra_cfg& c = h->cfg;
  const int R = c.heads * c.n_query;
  CrossPlan x{};
  x.precise = precise;
  x.probe = probe;
  // the folded form pays once the encoder sequence is long (fewer flops at any Kv, but five launches per layer); split precision and the
  // probe run only in it.  The streaming kernels (fold_stream.hip): f16 operands, 384 (head, query) rows, E a multiple of 176
  const bool fold = h->ncross > 0 && (precise || probe || h->cross_mode == 2 || (h->cross_mode == 0 && kv >= 2048));
  const bool stream = fold && !precise && !probe && h->fold_stream && fold_stream_supported(R, c.enc_width, kv, fold_kvp(kv), h->op());
  x.form = stream ? CrossPlan::FOLD_STREAM : fold ? CrossPlan::FOLD : CrossPlan::KV_CACHE;
  x.kmajor = R == 384 && c.enc_width % 176 == 0;   // the 176 x 384 loader-wave tile: one workgroup per CU at E = 1408
  x.softpart = R == 384;
  x.inreg = (h->inreg_rescale || probe) && x.softpart && x.kmajor;
  x.scores_tile = R == 384 ? GT_WS_176x384 : GT_128;
  x.penc_tile = x.kmajor ? GT_WS_176x384 : (R == 384 ? h->fold_tile : GT_128);
  // the default folded plan: the 176 x 384 tiles with in-register row factors, operand precision, no probe
  const bool default_fold = x.form == CrossPlan::FOLD && x.softpart && x.kmajor && x.inreg && !precise && !probe;
  x.raw = raw && default_fold;
  x.fuse_query = (h->cross_fuse & 1) && default_fold && c.hidden == c.heads * 64 && c.enc_width % 64 == 0;
  x.stat_factors = (h->cross_fuse & 2) && default_fold;
  x.ctx_64 = (h->cross_fuse & 4) && default_fold && c.enc_width % 128 == 0;
  return x;
}

// One lane's view of the workspace; with base == nullptr only measured.
struct Work {
  float *hA32, *hB32, *pre32, *hC32, *part;
  char *hA16, *hB16, *qkv16, *ctx16, *qc16, *hC16, *ffn16, *kv16;
  char *encT, *qp16, *p16, *u16;   // folded cross-attention: enc^T [N][E][kvp], Q' [N][R][E], P [N][R][kvp], U [N][R][E]
  char* qpb16;                     // streaming kernels: Q' in their blocked layout [N][R][E]
  char *hs16, *qs16;               // split-precision cross-attention: (hi | lo | hi) of the query rows [N*Q][3H] and of Q per head [N*Q][heads][192]
  float *qc32, *qp32;              // ... Q [N*Q][H] and Q' [N][R][E] in f32 (then Q' leaves as (hi | lo) rows [N][R][2E] in qp16)
  unsigned* lncnt;                 // fused residual + LayerNorm: one counter per 64-row tile and problem (zeroed at the start of a forward)
  size_t lncnt_bytes;
  float* s32;                      // scores [N][R][kvp]
  float* stat;                     // split softmax: tile maxima [N][R][ntiles], then tile sums
  float* gfac;                     // split softmax: row factors exp2(m_tile - m_row) / L as [N][ntiles][512] for the P . enc GEMM
  float* rt;                       // raw features: token factors 1 / sqrt(var + eps) [N][kvp], written by cross layer 0's scores launch
  float *st_m, *st_l, *ginv;       // streaming kernels: statistics [N * R][stat_ld], 1 / L [N * R]
  char* gexp;                      // tile factors f16 [N * R][stat_ld]
  int nsplit;
};

// One Q-Former of a forward: mra_qformer_forward runs one lane, mra_qformer_forward_pair two of equal shape.
struct Lane {
  mra_qformer* h;
  const void* enc;
  int kv;
  CrossPlan plan;
  const float* query;          // query tokens [1 or items][32][H] ...
  long long query_stride;      // ... and their item stride (0: shared)
  float *out_query, *out_full, *out_cls;
  Work w;
  int share = 1;               // chain items per encoder item (mra_qformer_forward_multi: the prompts of a clip); K/V-cache form only
};

// the layer chain's buffers for NN items (residual streams, QKV, attention context, feed-forward intermediate), seen from item n0 on
void layout_chain(Carver& cv, Work& w, size_t NN, size_t n0, size_t S, size_t H, size_t I, size_t Q) {
  auto f32 = [&](size_t per_item) { float* p = cv.take<float>(NN * per_item); return p ? p + n0 * per_item : p; };
  auto op = [&](size_t per_item) { char* p = cv.take<char>(NN * per_item, 2); return p ? p + n0 * per_item * 2 : p; };
  w.hA32 = f32(S * H);
  w.hB32 = f32(S * H);
  w.pre32 = f32(S * H);
  w.hC32 = f32(Q * H);
  w.hA16 = op(S * H);
  w.hB16 = op(S * H);
  w.qkv16 = op(S * 3 * H);
  w.ctx16 = op(S * H);
  w.qc16 = op(Q * H);
  w.hC16 = op(Q * H);
  w.ffn16 = op(S * I);
  w.lncnt_bytes = 2 * (NN * S / 64 + 2) * sizeof(unsigned);
  w.lncnt = cv.take<unsigned>(w.lncnt_bytes / sizeof(unsigned));
}

// one lane's cross-attention buffers for N encoder items (K/V cache, or the folded form's Q' / P / U / statistics), each read by
// `share` chain items
void layout_cross(const mra_qformer* h, const CrossPlan& x, Carver& cv, Work& w, int N, int Kv, int share = 1) {
  const mra_cfg& c = h->cfg;
  const size_t H = c.hidden, Q = c.n_query, E = c.enc_width, R = (size_t)c.heads * Q, kvp = fold_kvp(Kv);
  if (x.form == CrossPlan::FOLD_STREAM) {
    const size_t sld = fold_stream_stat_ld((int)kvp);
    w.qp16 = cv.take<char>((size_t)N * R * E, 2);
    w.qpb16 = cv.take<char>((size_t)N * R * E, 2);
    w.st_m = cv.take<float>((size_t)N * R * sld);
    w.st_l = cv.take<float>((size_t)N * R * sld);
    w.gexp = cv.take<char>((size_t)N * R * sld, 2);
    w.ginv = cv.take<float>((size_t)N * R);
    w.p16 = cv.take<char>((size_t)N * R * kvp, 2);
    w.u16 = cv.take<char>((size_t)N * R * E, 2);
  } else if (x.form == CrossPlan::FOLD) {
    if (!x.kmajor) w.encT = cv.take<char>((size_t)N * E * kvp, 2);
    w.qp16 = cv.take<char>((size_t)N * R * E * (x.precise ? 2 : 1), 2);
    if (x.precise) {
      w.hs16 = cv.take<char>((size_t)N * Q * 3 * H, 2);
      w.qs16 = cv.take<char>((size_t)N * Q * 3 * H, 2);
      w.qc32 = cv.take<float>((size_t)N * Q * H);
      w.qp32 = cv.take<float>((size_t)N * R * E);
    }
    if (!x.softpart) w.s32 = cv.take<float>((size_t)N * R * kvp);   // with softpart the scores never exist in fp32
    w.stat = cv.take<float>((size_t)2 * N * R * ((Kv + 175) / 176));
    if (x.inreg) w.gfac = cv.take<float>((size_t)N * ((Kv + 175) / 176) * 512);
    w.p16 = cv.take<char>((size_t)N * R * kvp, 2);
    w.u16 = cv.take<char>((size_t)N * R * E, 2);
    if (x.raw) w.rt = cv.take<float>((size_t)N * kvp);   // last: every other buffer sits where the normalised-copy form has it
  } else {
    w.kv16 = cv.take<char>((size_t)h->ncross * 2 * N * Kv * H, 2);
  }
  // which core runs a shared K/V stream: attn_kernel with kv_share at share == 1 (the existing forward, launch for launch) and
  // multi_core 0, the shared-stream core otherwise; each splits long KV by its own rule
  w.nsplit = share > 1 && h->multi_core == 1 ? attn_shared_pick_split(N, share, c.heads, Kv) : attn_pick_split(N * share, c.heads, (int)Q, Kv);
}

// The workspace of a forward over nl lanes of N items each; with base == nullptr only measures.  Returns its bytes.  The chain buffers hold
// nl N items (lane 0's, then lane 1's), so attention cores and LayerNorms take every lane in one launch and each chain GEMM groups the lanes'
// problems; behind them each lane's cross-attention buffers and grid-split attention partials, then (two lanes) the attention mask rows of both.
size_t layout_lanes(Lane* lanes, int nl, char* base, int N, int L, long long** mask2 = nullptr) {
  const mra_cfg& c = lanes[0].h->cfg;
  const size_t S = (size_t)c.n_query + L;
  Carver cv(base);
  const Carver chain = cv;
  for (int l = 0; l < nl; ++l) {
    lanes[l].w = Work{};
    cv = chain;
    layout_chain(cv, lanes[l].w, (size_t)nl * N, (size_t)l * N, S, c.hidden, c.inter, c.n_query);
  }
  for (int l = 0; l < nl; ++l) {
    Work& w = lanes[l].w;
    layout_cross(lanes[l].h, lanes[l].plan, cv, w, N / lanes[l].share, lanes[l].kv, lanes[l].share);
    // (the two-lane layout has always kept 64 floats of slack behind each lane's partials)
    float* part = cv.take<float>(attn_partial_bytes(N, c.heads, c.n_query, w.nsplit) / sizeof(float) + (nl > 1 ? 64 : 0));
    w.part = w.nsplit > 1 ? part : nullptr;
  }
  long long* m2 = nl > 1 ? cv.take<long long>((size_t)nl * N * S) : nullptr;
  if (mask2) *mask2 = m2;
  return cv.off;
}

// a lane of handle h over the encoder tokens enc (kv per item), its cross-attention planned for (precise, probe), no outputs yet
Lane make_lane(mra_qformer* h, const void* enc, int kv, bool precise, bool probe, bool raw = false) {
  Lane x{};
  x.h = h;
  x.enc = enc;
  x.kv = kv;
  x.plan = cross_plan(h, kv, precise, probe, raw);
  x.query = h->query;
  return x;
}

// workspace of a single-lane forward
size_t work_bytes(Lane x, int N, int L) { return layout_lanes(&x, 1, nullptr, N, L); }

// Steps 6 / 6a-6e of one cross-attention layer of one lane: from the query projection Q (w.qc16, or w.qc32 in split precision) to the
// attention context (w.ctx16 [N*Q][H]) -- the folded form (per-head Q' GEMM, scores + split softmax, P . enc, per-head context GEMM) or the
// core over the head-major K/V cache.  With CrossPlan::fuse_query step 6a has already run, fused into the query projection (run_lanes).
int cross_core(const Lane& lane, const LayerW& Lw, int N, hipStream_t stream) {
  const mra_qformer* h = lane.h;
  const CrossPlan& x = lane.plan;
  const Work& w = lane.w;
  const void* enc = lane.enc;
  const int kv = lane.kv;
  const mra_cfg& c = h->cfg;
  const int Q = c.n_query, H = c.hidden, E = c.enc_width, R = c.heads * Q, kvp = fold_kvp(kv), op = h->op();
  const size_t esz = 2;
  const RowView qc_rows = plain(N * Q, H);
  const int ci = Lw.cross_index;
  int rc = 0;
  if (x.form == CrossPlan::KV_CACHE) {
    // 6. cross-attention core over the head-major K/V cache
    // (the cache holds N / share encoder items; chain item n reads the K/V of item n / share)
    AttnArgs a = kv_cross_attn_args(c, w.qc16, w.kv16, ci, w.ctx16, N / lane.share, kv, w.nsplit, w.part);
    a.items = N;
    a.kv_share = lane.share;
    rc = lane.share > 1 && h->multi_core == 1 ? launch_attention_shared(a, op, stream) : launch_attention(a, op, stream);
    return rc ? chk(rc, "cross attention") : MRA_OK;
  }
  const bool timed = ci == 0 && h->kv_ev0 && h->kv_ev1;
  if (timed && !x.fuse_query) (void)hipEventRecord(h->kv_ev0, stream);   // (fused: run_lanes recorded it in front of step 6a)
  int* hist = x.probe ? h->auto_hist + (size_t)ci * 256 : nullptr;
  // 6a. Q' = Q_h W_k,h per head: [N*32, 64] x [E, 64]^T -> Q' [N][head*32 + q][E]
  GemmProb d{};
  if (x.precise) {
    // Q (fp32) per head as (hi | lo | hi) over its 64 dims against W_k,h as (hi | hi | lo): K = 192; Q' in fp32, then as (hi | lo) rows
    rc = launch_split_rows(w.qc32, qc_rows, N * Q, H, 64, 3, w.qs16, op, stream);
    if (rc) return chk(rc, "split cross query");
    d.A = w.qs16; d.a = plain(N * Q, 3 * H); d.a_bs = 192;
    d.W = h->arena_p + (size_t)ci * precise_layer_bytes(h) + precise_wk_off(h); d.w_bs = (long long)E * 192;
    d.C = w.qp32; d.c = items_view((long long)R * E, Q, E); d.c_bs_bytes = (long long)Q * E * 4;
    d.M = N * Q; d.N = E; d.K = 192; d.batch = c.heads; d.tile_cfg = (N * Q) % 128 == 0 && E % 128 == 0 ? GT_128 : GT_64;
    rc = launch_gemm(&d, 1, EPI_F32, op, stream);
    if (rc) return chk(rc, "fold q' gemm (split precision)");
    rc = launch_split_rows(w.qp32, plain(N * R, E), N * R, E, E, 2, w.qp16, op, stream);
    if (rc) return chk(rc, "split q'");
  } else if (!x.fuse_query) {   // (fused: run_lanes wrote Q' together with the query projection)
    d.A = w.qc16; d.a = qc_rows; d.a_bs = 64;
    d.W = x.raw ? fold_raw_wk(h, ci) : h->arena_f + (size_t)ci * H * E * esz; d.w_bs = (long long)E * 64;
    d.C = w.qp16; d.c = items_view((long long)R * E, Q, E); d.c_bs_bytes = (long long)Q * E * esz;
    d.M = N * Q; d.N = E; d.K = 64; d.batch = c.heads; d.tile_cfg = (N * Q) % 128 == 0 && E % 128 == 0 ? GT_128 : GT_64;
    rc = launch_gemm(&d, 1, EPI_OP, op, stream);
    if (rc) return chk(rc, "fold q' gemm");
  }
  if (x.form == CrossPlan::FOLD_STREAM) {
    // 6b-6d on the streaming kernels (fold_stream.hip): P~ = exp2(s - ceil(tile max)) + tile statistics, row statistics,
    // U = (1 / L) sum g P~ enc with the power-of-two tile factors applied in registers.  P~ is written once, read once.
    FoldStreamArgs fs{};
    fs.qp = w.qp16; fs.qpb = w.qpb16; fs.enc = enc; fs.p = w.p16; fs.u = w.u16;
    fs.stat_m = w.st_m; fs.stat_l = w.st_l; fs.gexp = w.gexp; fs.ginv = w.ginv;
    fs.items = N; fs.kv = kv; fs.kvp = kvp; fs.E = E;
    fs.alpha = 0.125f * 1.4426950408889634f; fs.phase = 3;
    rc = launch_fold_stream(fs, stream);
    if (rc) return chk(rc, "fold scores / P.enc (streaming kernels)");
  } else {
    // 6b. scores S[n] = Q'[n] enc[n]^T: [R, E] x [kv, E]^T per item, rows padded to kvp columns
    GemmProb sc{};
    sc.A = w.qp16; sc.a = plain(R, E); sc.a_bs = (long long)R * E;
    sc.W = enc; sc.w_bs = (long long)kv * E;
    sc.M = R; sc.N = kv; sc.K = E; sc.batch = N; sc.n_ragged = 1;
    if (x.precise) {   // Q' rows are (hi | lo): two passes over the same encoder slab inside one K loop
      sc.a = plain(R, 2 * E); sc.a_bs = (long long)R * 2 * E; sc.K = 2 * E; sc.w_kwrap = E / 64;
    }
    sc.tile_cfg = x.scores_tile;
    const int ntiles = (kv + 175) / 176;
    if (x.softpart) {
      // 6b + 6c fused: the GEMM's epilogue leaves exp2(s - tile maximum) in the operand dtype plus tile statistics;
      // one pass over P rescales every row by exp2(m_tile - m_row) / sum.  The scores never exist in fp32 in HBM.
      sc.C = w.p16; sc.c = plain(R, kvp); sc.c_bs_bytes = (long long)R * kvp * esz;
      sc.alpha = 0.125f * 1.4426950408889634f;
      sc.stat_m = w.stat; sc.stat_l = w.stat + (size_t)N * R * ntiles;
      if (x.raw) {   // raw tokens: column t carries r_t; the first cross layer computes the factors as the tokens stream through its LDS
        sc.col_scale = w.rt; sc.cs_bs = kvp; sc.col_stats = ci == 0; sc.cs_eps = c.enc_ln_eps;
      }
      rc = launch_gemm(&sc, 1, EPI_SOFTPART, op, stream);
      if (rc) return chk(rc, "fold scores gemm (softmax partials)");
      if (x.stat_factors) {
        // the P . enc launch computes the row factors itself from these statistics (and zeroes the unwritten P~ columns in its LDS)
      } else if (x.inreg) {
        // second half of the softmax without a pass over P: only the row factors are computed here, the P . enc GEMM applies them
        // to its P~ fragments in registers (same arithmetic, same rounding as the rescale pass)
        rc = launch_fold_rowfactor(sc.stat_m, sc.stat_l, w.gfac, N * R, R, ntiles, w.p16, kvp, 176, kvp, stream, hist);
        if (rc) return chk(rc, "fold row factors");
      } else {
        rc = launch_softmax_rescale(w.p16, kvp, sc.stat_m, sc.stat_l, N * R, ntiles, 176, kvp, op, stream, hist);
        if (rc) return chk(rc, "fold softmax rescale");
      }
    } else {
      sc.C = w.s32; sc.c = plain(R, kvp); sc.c_bs_bytes = (long long)R * kvp * 4;   // fp32 rows
      rc = launch_gemm(&sc, 1, EPI_F32, op, stream);
      if (rc) return chk(rc, "fold scores gemm");
      // 6c. P = softmax(S / 8) row by row (the key bias is constant along a row and cancels)
      rc = launch_softmax_rows(w.s32, kvp, w.p16, kvp, N * R, kv, kvp, 0.125f, op, stream);
      if (rc) return chk(rc, "fold softmax");
    }
    // 6d. U[n] = P[n] enc[n]: [R, kvp] x [E, kvp]^T per item
    GemmProb pv{};
    pv.A = w.p16; pv.a = plain(R, kvp); pv.a_bs = (long long)R * kvp;
    if (x.kmajor) {   // the encoder tokens themselves: [kv][E] is W K-major; rows kv .. kvp repeat the last token against P = 0
      pv.W = enc; pv.w_bs = (long long)kv * E; pv.w_ld = E; pv.k_rows = kv;
    } else {
      pv.W = w.encT; pv.w_bs = (long long)E * kvp;
    }
    pv.C = w.u16; pv.c = plain(R, E); pv.c_bs_bytes = (long long)R * E * esz;
    pv.M = R; pv.N = E; pv.K = kvp; pv.batch = N;
    pv.tile_cfg = x.penc_tile;
    if (x.stat_factors) { pv.stat_m = sc.stat_m; pv.stat_l = sc.stat_l; pv.ps_stats = 1; pv.ps_ntiles = ntiles; }
    else if (x.inreg) { pv.pscale = w.gfac; pv.ps_ntiles = ntiles; }
    rc = launch_gemm(&pv, 1, EPI_OP, op, stream);
    if (rc) return chk(rc, "fold p.enc gemm");
  }
  // 6e. context = U_h W_v,h^T + b_v,h per head: [N*32, E] x [64, E]^T -> ctx [N*32][head*64 + d]
  GemmProb cx{};
  cx.A = w.u16; cx.a = items_view((long long)R * E, Q, E); cx.a_bs = (long long)Q * E;
  cx.W = (const char*)h->wkv + (size_t)(ci * 2 + 1) * H * E * esz; cx.w_bs = (long long)64 * E;
  cx.bias = h->bkv + (size_t)(ci * 2 + 1) * H; cx.bias_bs = 64;
  if (x.raw) { cx.W = fold_raw_wv(h, ci); cx.bias = fold_raw_bv(h, ci); }   // U is over raw tokens: W_v' and b_v + W_v b
  cx.C = w.ctx16; cx.c = qc_rows; cx.c_bs_bytes = 64 * esz;
  cx.M = N * Q; cx.N = 64; cx.K = E; cx.batch = c.heads; cx.tile_cfg = E % 128 == 0 && N * Q >= 512 ? GT_K128_64x128 : GT_64;
  if (x.ctx_64 && cx.tile_cfg == GT_K128_64x128) { cx.tile_cfg = GT_64; cx.k128 = 1; }
  rc = launch_gemm(&cx, 1, EPI_OP, op, stream);
  if (rc) return chk(rc, "fold context gemm");
  if (timed) (void)hipEventRecord(h->kv_ev1, stream);
  return MRA_OK;
}

}  // namespace

namespace mra_host {
// K/V of every cross layer in ONE GEMM: [items*kv, E] x [ncross*2*H, E]^T, scattered head-major.
int kv_project(const mra_qformer* h, const void* enc, int N, int kv, void* kv_cache, hipStream_t stream) {
  const mra_cfg& c = h->cfg;
  GemmProb p{};
  p.A = enc;
  p.a = plain(N * kv, c.enc_width);
  p.W = h->wkv;
  p.bias = h->bkv;
  p.C = kv_cache;
  p.c = plain(1, 1);
  p.M = N * kv;
  p.N = h->ncross * 2 * c.hidden;
  p.K = c.enc_width;
  p.kv_tokens = kv;
  p.kv_items = N;
  p.kv_heads = c.heads;
  p.persist = 1;   // on the eight-phase kernel: one persistent workgroup per CU (bit-identical; no workgroup turnaround between tiles)
  return launch_gemm(&p, 1, EPI_KV, h->op(), stream);
}

}  // namespace mra_host

extern "C" {

const char* mra_last_error(void) { return g_err.c_str(); }
const char* mra_version(void) { return "mraudio_amd 0.1 (gfx950)"; }
int64_t mra_debug_gemm_launches(int32_t family, int32_t epilogue) { return gemm_launch_count(family, epilogue); }

void mra_cfg_default(mra_cfg* c, int32_t enc_width) {
  c->hidden = 768;
  c->heads = 12;
  c->inter = 3072;
  c->layers = 12;
  c->cross_freq = 2;
  c->enc_width = enc_width;
  c->n_query = 32;
  c->vocab = 30523;
  c->max_pos = 512;
  c->ln_eps = 1e-12f;
  c->enc_ln_eps = 1e-5f;
  c->llm_hidden = 4096;
  c->op_dtype = MRA_F16;
}

int mra_qformer_create(const mra_cfg* cfg, mra_qformer** out) {
  if (!cfg || !out) return fail(MRA_EINVAL, "null argument");
  const mra_cfg& c = *cfg;
  if (c.hidden <= 0 || c.hidden % 256 || c.hidden > 1024) return fail(MRA_EINVAL, "hidden must be a multiple of 256, <= 1024");
  if (c.heads <= 0 || c.hidden != c.heads * 64) return fail(MRA_EINVAL, "head_dim must be 64");
  if (c.n_query != 32) return fail(MRA_EINVAL, "n_query must be 32");
  if (c.inter <= 0 || c.inter % 256) return fail(MRA_EINVAL, "inter must be a multiple of 256");
  if (c.enc_width <= 0 || c.enc_width % 64) return fail(MRA_EINVAL, "enc_width must be a multiple of 64");
  if (c.layers <= 0 || c.cross_freq <= 0 || c.vocab <= 0 || c.max_pos <= 0) return fail(MRA_EINVAL, "bad layer/vocab config");
  if (c.llm_hidden < 0 || c.llm_hidden % 64) return fail(MRA_EINVAL, "llm_hidden must be 0 or a multiple of 64");
  if (c.op_dtype != MRA_F16 && c.op_dtype != MRA_BF16) return fail(MRA_EINVAL, "op_dtype must be MRA_F16 or MRA_BF16");
  mra_qformer* h = new mra_qformer();
  h->cfg = c;
  HIP_TRY(hipGetDevice(&h->device));
  h->arena_bytes = layout_params(h, nullptr);
  hipError_t e = hipMalloc((void**)&h->arena, h->arena_bytes);
  if (e != hipSuccess) {
    delete h;
    return fail(MRA_ENOMEM, std::string("hipMalloc of parameter arena: ") + hipGetErrorString(e));
  }
  layout_params(h, h->arena);
  if (h->ncross > 0) {
    e = hipMalloc((void**)&h->arena_f, fold_arena_bytes(h));
    if (e != hipSuccess) {
      mra_qformer_destroy(h);
      return fail(MRA_ENOMEM, std::string("fold weight arena: ") + hipGetErrorString(e));
    }
  }
  // segment table of mra_qformer_load_flat: every bert.* parameter in chunks of FLAT_SEG elements
  std::vector<FlatSeg> segs;
  for (auto& kv : h->params) {
    if (kv.first.rfind("bert.", 0) != 0) continue;
    const Param& pr = kv.second;
    const size_t esz = pr.dtype == MRA_F32 ? 4 : 2;
    for (long long o = 0; o < pr.numel; o += FLAT_SEG)
      segs.push_back(FlatSeg{(unsigned long long)(pr.goff / 4 + o), (char*)pr.ptr + o * esz,
                             (int)std::min<long long>(FLAT_SEG, pr.numel - o), pr.dtype});
    if (pr.copy32)   // the f32 copies of the score-chain weights follow the master too
      for (long long o = 0; o < pr.numel; o += FLAT_SEG)
        segs.push_back(FlatSeg{(unsigned long long)(pr.goff / 4 + o), (char*)(pr.copy32 + o), (int)std::min<long long>(FLAT_SEG, pr.numel - o), MRA_F32});
  }
  h->n_flat_segs = (int)segs.size();
  e = hipMalloc((void**)&h->flat_segs, segs.size() * sizeof(FlatSeg));
  if (e == hipSuccess) e = hipMemcpy(h->flat_segs, segs.data(), segs.size() * sizeof(FlatSeg), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    mra_qformer_destroy(h);
    return fail(MRA_ENOMEM, std::string("segment table: ") + hipGetErrorString(e));
  }
  *out = h;
  return MRA_OK;
}

void mra_qformer_destroy(mra_qformer* h) {
  if (!h) return;
  if (h->arena) (void)hipFree(h->arena);
  if (h->arena_t) (void)hipFree(h->arena_t);
  if (h->arena_f) (void)hipFree(h->arena_f);
  if (h->arena_p) (void)hipFree(h->arena_p);
  if (h->auto_hist) (void)hipFree(h->auto_hist);
  if (h->auto_hist_host) (void)hipHostFree(h->auto_hist_host);
  if (h->flat_segs) (void)hipFree(h->flat_segs);
  if (h->tr_jobs) (void)hipFree(h->tr_jobs);
  if (h->adam_jobs) (void)hipFree(h->adam_jobs);
  if (h->adam_segs) (void)hipFree(h->adam_segs);
  if (h->c32_segs) (void)hipFree(h->c32_segs);
  for (auto& e : h->wg_ev) if (e) (void)hipEventDestroy(e);
  if (h->wg_stream) (void)hipStreamDestroy(h->wg_stream);
  delete h;
}

int mra_qformer_load(mra_qformer* h, const char* name, const void* src, int32_t dtype, const int64_t* shape,
                     int32_t ndim, void* stream) {
  if (!h || !name || !src || (ndim > 0 && !shape)) return fail(MRA_EINVAL, "null argument");
  if (dtype < MRA_F32 || dtype > MRA_BF16) return fail(MRA_EINVAL, "bad dtype");
  const std::string key(name);
  if (key == "bert.embeddings.position_ids") return MRA_OK;  // LAVIS buffer, not a parameter
  auto it = h->params.find(key);
  if (it == h->params.end()) return fail(MRA_ENAME, "unknown parameter name: " + key);
  long long numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= shape[i];
  if (numel != it->second.numel)
    return fail(MRA_EINVAL, "parameter " + key + ": expected " + std::to_string(it->second.numel) + " elements, got " +
                                std::to_string(numel));
  int rc = launch_convert(src, dtype, it->second.ptr, it->second.dtype, numel, as_stream(stream));
  if (!rc && it->second.copy32) rc = launch_convert(src, dtype, it->second.copy32, MRA_F32, numel, as_stream(stream));
  if (rc) return chk(rc, "launch_convert");
  it->second.loaded = true;
  h->transposes_stale = true;
  h->fold_stale = true;
  h->precise_stale = true;
  h->auto_stale = true;
  return MRA_OK;
}

int mra_qformer_load_flat(mra_qformer* h, const float* master, size_t master_bytes, void* stream) {
  if (!h || !master) return fail(MRA_EINVAL, "null argument");
  if (master_bytes < h->grad_bytes) return fail(MRA_EINVAL, "master buffer smaller than mra_qformer_grad_bytes()");
  if ((size_t)master & 15) return fail(MRA_EINVAL, "master buffer must be 16-byte aligned");
  const int rc = launch_convert_flat(master, h->flat_segs, h->n_flat_segs, as_stream(stream));
  if (rc) return chk(rc, "launch_convert_flat");
  for (auto& kv : h->params)
    if (kv.first.rfind("bert.", 0) == 0) kv.second.loaded = true;
  h->transposes_stale = true;
  h->fold_stale = true;
  h->precise_stale = true;
  h->auto_stale = true;
  return MRA_OK;
}

int mra_qformer_missing(mra_qformer* h, char* buf, size_t buflen) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  int n = 0;
  std::string s;
  for (auto& kv : h->params)
    if (!kv.second.loaded) {
      ++n;
      if (!s.empty()) s += ",";
      s += kv.first;
    }
  if (buf && buflen) {
    std::strncpy(buf, s.c_str(), buflen - 1);
    buf[buflen - 1] = 0;
  }
  return n;
}

int mra_modality_ln(mra_qformer* h, const void* x, int32_t x_dtype, const int64_t* item_index, int32_t items,
                    int32_t tokens, void* out, void* stream) {
  if (!h || (!x && items > 0) || (!out && items > 0)) return fail(MRA_EINVAL, "null argument");
  if (items < 0 || tokens < 0) return fail(MRA_EINVAL, "negative size");
  if (items == 0 || tokens == 0) return MRA_OK;
  if (!h->params["ln.weight"].loaded || !h->params["ln.bias"].loaded) return fail(MRA_ESTATE, "ln.weight / ln.bias not loaded");
  return chk(launch_modality_ln(x, x_dtype, (const long long*)item_index, items, tokens, h->cfg.enc_width, h->encg,
                                h->encb, h->cfg.enc_ln_eps, out, h->op(), as_stream(stream)),
             "modality_ln");
}

int mra_modality_ln_backward(mra_qformer* h, const void* x, int32_t x_dtype, int32_t items, int32_t tokens, const float* d_out, float* d_x,
                             float* d_gain, float* d_bias, void* stream) {
  if (items < 0 || tokens < 0) return fail(MRA_EINVAL, "negative size");
  if (x_dtype != MRA_F32 && x_dtype != MRA_F16 && x_dtype != MRA_BF16) return fail(MRA_EINVAL, "x_dtype must be f32, f16 or bf16");
  if (items > 0 && tokens > 0 && (!x || !d_out)) return fail(MRA_EINVAL, "null x or d_out");
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (items == 0 || tokens == 0) return MRA_OK;
  if (!h->params["ln.weight"].loaded || !h->params["ln.bias"].loaded) return fail(MRA_ESTATE, "ln.weight / ln.bias not loaded");
  return chk(launch_modality_ln_bwd(x, x_dtype, items, tokens, h->cfg.enc_width, h->encg, h->cfg.enc_ln_eps, d_out, d_x, d_gain, d_bias,
                                    as_stream(stream)),
             "modality_ln backward");
}

size_t mra_qformer_workspace_bytes(mra_qformer* h, int32_t items, int32_t L, int32_t kv) {
  if (!h || items <= 0 || L < 0 || kv <= 0) return 0;
  // (a raw-feature forward adds its token factors behind the other buffers: asked for whenever that form could run)
  if (!h->cross_auto) return work_bytes(make_lane(h, nullptr, kv, h->cross_precise, false, true), items, L);
  // automatic precision: the largest of op, the probing forward's op-precision folded form and split precision, so neither the probe nor
  // its resolution ever needs a larger workspace
  return std::max({work_bytes(make_lane(h, nullptr, kv, false, false, true), items, L), work_bytes(make_lane(h, nullptr, kv, false, true), items, L),
                   work_bytes(make_lane(h, nullptr, kv, true, false), items, L)});
}

double mra_qformer_flops(mra_qformer* h, int32_t items, int32_t L, int32_t kv, int32_t with_last_text) {
  if (!h) return 0.0;
  const mra_cfg& c = h->cfg;
  const double H = c.hidden, I = c.inter, E = c.enc_width, Q = c.n_query, S = Q + L, Kv = kv;
  double per_item = c.layers * (8 * S * H * H + 4 * S * S * H + 4 * S * H * I) +
                    h->ncross * (4 * Q * H * H + 4 * Kv * E * H + 4 * Q * Kv * H);
  if (!with_last_text) per_item -= 4.0 * L * H * I;
  return per_item * items;
}

namespace {
// every parameter loaded, except the optional modality LayerNorm (ln.*) and LLM projection (llm_proj.*)
int check_loaded(mra_qformer* h) {
  char names[256];
  const int miss = mra_qformer_missing(h, names, sizeof(names));
  int tolerated = 0;
  for (const char* opt : {"ln.weight", "ln.bias", "llm_proj.weight", "llm_proj.bias"}) {
    auto it = h->params.find(opt);
    if (it != h->params.end() && !it->second.loaded) ++tolerated;
  }
  return miss > tolerated ? fail(MRA_ESTATE, std::string("parameters not loaded: ") + names) : MRA_OK;
}

// Steps 1 + 2 of every layer in one launch (launch_qkv_attention) instead of two: the option, a single lane, S <= 64 and 64-wide heads (H is
// then a multiple of the 64-deep K step; the operand dtype of a handle is always f16 or bf16) -- and a forward whose QKV GEMM would run its
// ring tile (chain_ring bit 0, >= 1024 rows, 3 H a multiple of 144).  The fused launch adds the ring kernel's two accumulator chains (even and
// odd K tiles), the two-buffer tiles of smaller forwards ONE chain over K: with the last condition the option never changes a bit of any
// forward, so the pair forward and the single-lane forwards stay equal at every size.  A forward that returns the full sequence (out_full: the
// reference-style call, not the scoring path) keeps the launch sequence that "chain_ring" alone selects -- tests/test_gpu_parity.py counts its
// QKV ring launches per mask.  Everything else keeps the two launches.
bool self_fuse_plan(int option, int lanes, long long rows, int S, int hidden, int heads, int op, int chain_ring, bool want_full) {
  return option == 1 && lanes == 1 && !want_full && (op == OP_F16 || op == OP_BF16) && qkv_attn_supported(S, hidden, heads) && (chain_ring & 1) && rows >= 1024 &&
         (3 * hidden) % 144 == 0;
}

// The Q-Former forward of nl lanes (1: mra_qformer_forward, 2: mra_qformer_forward_pair) of N items with L text rows: embeddings, the
// layers, the last layer's LayerNorms into the lanes' outputs.  A grouped launch holds the query problems of every lane, then their text
// problems.  Split precision, out_full, query_embeds and the fused residual + LayerNorm (chain_ring bit 3) are single-lane only.
int run_lanes(Lane* lanes, int nl, const int64_t* input_ids, const int64_t* attention_mask, int N, int L, void* workspace, hipStream_t stream) {
  const mra_qformer* h = lanes[0].h;   // the lanes agree in hidden / heads / inter / layers / cross_freq / n_query / op dtype / ln_eps
  const mra_cfg& c = h->cfg;
  const bool pair = nl == 2;
  const int Q = c.n_query, S = Q + L, H = c.hidden, I = c.inter;
  const int op = h->op();
  long long* mask2 = nullptr;
  layout_lanes(lanes, nl, (char*)workspace, N, L, &mask2);
  const Work& w = lanes[0].w;   // the chain buffers of every lane, lane 0's first
  const long long SH = (long long)S * H;
  const size_t esz = 2;

  // row views of the [N, S, H] streams
  const RowView all_rows = plain(N * S, H), all_lanes = plain(nl * N * S, H);
  const RowView q_view = items_view(SH, Q, H);              // rows [:, :32]
  const RowView t_view = items_view(SH, L > 0 ? L : 1, H);  // rows [:, 32:] (base pointer + 32*H)
  const RowView cls_view = items_view(SH, 1, H);            // row  [:, 32]
  const RowView qc_rows = plain(N * Q, H);                  // compact [N*32, H]
  const size_t t_off16 = (size_t)Q * H * esz;               // byte offset of row 32 inside an item (op dtype)
  const size_t t_off32 = (size_t)Q * H;                     // element offset (f32)

  // residual projection + LayerNorm in ONE launch (chain_ring bit 3, on the 96 x 64 ring tile): its per-row-tile counters start at zero
  const bool self_fuse = self_fuse_plan(h->self_fuse, nl, (long long)N * S, S, H, c.heads, op, h->chain_ring, lanes[0].out_full != nullptr);
  const bool ln_fuse = !pair && (h->chain_ring & 12) == 12 && H % 96 == 0 && H % 256 == 0 && H <= 1024;
  int rc;
  for (int l = 0; l < nl; ++l) {
    Lane& x = lanes[l];
    mra_qformer* hl = x.h;
    rc = launch_embed_ln((const long long*)input_ids, N, L, Q, H, hl->cfg.vocab, x.query, x.query_stride, hl->word, hl->pos, hl->embg, hl->embb,
                         c.ln_eps, x.w.hA32, x.w.hA16, nullptr, op, stream);
    if (rc) return chk(rc, "embed_ln");
    if (ln_fuse) HIP_TRY(hipMemsetAsync(w.lncnt, 0, w.lncnt_bytes, stream));
    if (x.plan.form != CrossPlan::KV_CACHE) {
      // folded cross-attention: enc^T per item (the K-contiguous operand of P . enc), key weights regrouped per head
      if (x.plan.form == CrossPlan::FOLD && !x.plan.kmajor) {
        const int E = hl->cfg.enc_width, kvp = fold_kvp(x.kv);
        rc = launch_transpose_pad(x.enc, x.w.encT, x.kv, E, kvp, (long long)x.kv * E, (long long)E * kvp, N, op, stream);
        if (rc) return chk(rc, "enc transpose");
      }
      if ((rc = mra_qformer_prepare(hl, stream))) return rc;
    } else if (hl->ncross > 0) {
      // K/V of every cross layer in one GEMM, scattered head-major
      const bool timed = !pair && hl->kv_ev0 && hl->kv_ev1;
      if (timed) (void)hipEventRecord(hl->kv_ev0, stream);
      rc = kv_project(hl, x.enc, N / x.share, x.kv, x.w.kv16, stream);
      if (rc) return chk(rc, "kv projection gemm");
      if (timed) (void)hipEventRecord(hl->kv_ev1, stream);
    }
    if (!pair && hl->kv_done) (void)hipEventRecord(hl->kv_done, stream);   // also without cross layers: the waiter must not hang
  }
  const long long* mask = (const long long*)attention_mask;
  if (pair && mask) {   // the two lanes share the prompt: their mask rows one after the other for the 2 N-item attention launch
    HIP_TRY(hipMemcpyAsync(mask2, mask, (size_t)N * S * 8, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipMemcpyAsync(mask2 + (size_t)N * S, mask, (size_t)N * S * 8, hipMemcpyDeviceToDevice, stream));
    mask = mask2;
  }

  const bool want_text_last = lanes[0].out_full != nullptr;
  bool want_cls_last = false;
  for (int l = 0; l < nl; ++l) want_cls_last |= !want_text_last && lanes[l].out_cls;

  // Tile choice: the grouped launch runs the tile of its first problem.  The QKV and attention-output problems each take their own lane's
  // chain_ring mask, the feed-forward launches lane 0's.
  for (int i = 0; i < c.layers; ++i) {
    // Lw[l]: lane l's weights; the LayerNorm launches take lane 1's parameters from Lw[1] (lane 0's own in a single-lane forward, where
    // no row reaches lane_rows)
    const LayerW* Lw[2] = {&lanes[0].h->layers[i], &lanes[nl - 1].h->layers[i]};
    const bool last = i == c.layers - 1;
    if (self_fuse) {
      // 1 + 2. Q|K|V projection and self-attention core in one launch: Q, K, V pass through LDS, qkv16 is neither written nor read
      rc = launch_qkv_attention(w.hA16, Lw[0]->wqkv, Lw[0]->bqkv, mask, w.ctx16, N, S, H, c.heads, op, stream);
      if (rc) return chk(rc, "qkv + self attention");
    } else {
      // 1. fused Q|K|V projection of all S rows
      {
        GemmProb p[2] = {};
        for (int l = 0; l < nl; ++l) {
          p[l].A = lanes[l].w.hA16; p[l].a = all_rows;
          p[l].W = Lw[l]->wqkv; p[l].bias = Lw[l]->bqkv;
          p[l].C = lanes[l].w.qkv16; p[l].c = plain(N * S, 3 * H);
          p[l].M = N * S; p[l].N = 3 * H; p[l].K = H;
          // The chain GEMMs at ~1-2 k rows are bound by the operand bytes each CU pulls through its load path (~33 B / clk from L2),
          // not by tile count: 128 x 128 tiles (288 of them) move half the bytes per flop of the 1152 64 x 64 tiles the automatic
          // choice makes (headline step 6.75 -> 6.67 ms, reference item shape 2.65 -> 2.55 ms together with the down-projection below)
          p[l].tile_cfg = N * S >= 1024 ? GT_128 : GT_AUTO;
          // ... and at ~2 k rows the ring kernel's 144 x 128 tile is exactly one workgroup per CU (2048 x 2304 = 16 x 16 tiles): 14.4 vs 17.6 us stand-alone
          if ((lanes[l].h->chain_ring & 1) && N * S >= 1024 && (3 * H) % 144 == 0) p[l].tile_cfg = GT_RING_144x128;
        }
        rc = launch_gemm(p, nl, EPI_OP, op, stream);
        if (rc) return chk(rc, "qkv gemm");
      }
      // 2. self-attention core of all nl N items
      rc = launch_attention(self_attn_args(c, w.qkv16, w.ctx16, mask, nl * N, S), op, stream);
      if (rc) return chk(rc, "self attention");
    }
    // 3. output projection + residual, 4. LayerNorm -> hB
    {
      GemmProb p[2] = {};
      for (int l = 0; l < nl; ++l) {
        p[l].A = lanes[l].w.ctx16; p[l].a = all_rows;
        p[l].W = Lw[l]->wo; p[l].bias = Lw[l]->bo;
        p[l].R = lanes[l].w.hA32; p[l].r = all_rows;
        p[l].C = lanes[l].w.pre32; p[l].c = all_rows;
        p[l].M = N * S; p[l].N = H; p[l].K = H;
        if ((lanes[l].h->chain_ring & 4) && N * S >= 1024 && H % 96 == 0) p[l].tile_cfg = GT_RING_96x64;
      }
      if (ln_fuse && p[0].tile_cfg == GT_RING_96x64) {
        // HF:519-530 in one launch: the column tile of a 64-row block that finishes last normalises the block's rows
        p[0].ln_gain = Lw[0]->ln1g; p[0].ln_bias = Lw[0]->ln1b; p[0].ln_eps = c.ln_eps;
        p[0].ln_y32 = w.hB32; p[0].ln_y32v = all_rows; p[0].ln_y16 = w.hB16; p[0].ln_y16v = all_rows; p[0].ln_counter = w.lncnt;
        rc = launch_gemm(p, 1, EPI_RES_LN, op, stream);
        if (rc) return chk(rc, "attn out gemm + ln");
      } else {
        rc = launch_gemm(p, nl, EPI_RES_F32, op, stream);
        if (rc) return chk(rc, "attn out gemm");
        rc = launch_ln_rows4(w.pre32, all_lanes, nl * N * S, H, Lw[0]->ln1g, Lw[0]->ln1b, nullptr, nullptr, N * S, Lw[1]->ln1g, Lw[1]->ln1b, nullptr,
                             nullptr, 1, 1, c.ln_eps, w.hB32, all_lanes, w.hB16, all_lanes, op, stream);
        if (rc) return chk(rc, "attn ln");
      }
    }
    // query-side state entering the feed-forward: hB[:, :32] or the cross-attention output hC
    const bool cross = Lw[0]->cross_index >= 0;
    const RowView fqv = cross ? qc_rows : q_view;
    if (cross) {
      // 5. cross query projection
      if (lanes[0].plan.precise) {
        // split precision: the fp32 query rows leave as (hi | lo | hi), the weight is stored as (hi | hi | lo): one GEMM over K = 3H
        // computes xh wh + xl wh + xh wl in the fp32 accumulators; Q stays fp32
        rc = launch_split_rows(w.hB32, q_view, N * Q, H, H, 3, w.hs16, op, stream);
        if (rc) return chk(rc, "split query rows");
        GemmProb p{};
        p.A = w.hs16; p.a = plain(N * Q, 3 * H);
        p.W = h->arena_p + (size_t)Lw[0]->cross_index * precise_layer_bytes(h); p.bias = Lw[0]->bcq;
        p.C = w.qc32; p.c = qc_rows;
        p.M = N * Q; p.N = H; p.K = 3 * H;
        rc = launch_gemm(&p, 1, EPI_F32, op, stream);
      } else {
        // lanes whose plan fuses steps 5 + 6a write Q' here (Q itself has no other reader in that plan); the others share one grouped GEMM
        GemmProb p[2] = {};
        int ng = 0;
        rc = 0;
        for (int l = 0; l < nl && !rc; ++l) {
          const Lane& x = lanes[l];
          if (x.plan.fuse_query) {
            const int ci = Lw[l]->cross_index, E = x.h->cfg.enc_width;
            const void* wk = x.plan.raw ? fold_raw_wk(x.h, ci) : x.h->arena_f + (size_t)ci * H * E * esz;
            // the timed block of cross layer 0 keeps meaning steps 6a-6e: here it opens in front of the launch that holds 6a (and step 5)
            if (ci == 0 && x.h->kv_ev0 && x.h->kv_ev1) (void)hipEventRecord(x.h->kv_ev0, stream);
            rc = launch_fold_query(x.w.hB16, q_view, Lw[l]->wcq, Lw[l]->bcq, wk, x.w.qp16, N * Q, H, E, Q, c.heads, op, stream);
            continue;
          }
          p[ng].A = x.w.hB16; p[ng].a = q_view;
          p[ng].W = Lw[l]->wcq; p[ng].bias = Lw[l]->bcq;
          p[ng].C = x.w.qc16; p[ng].c = qc_rows;
          p[ng].M = N * Q; p[ng].N = H; p[ng].K = H;
          ++ng;
        }
        if (!rc && ng) rc = launch_gemm(p, ng, EPI_OP, op, stream);
      }
      if (rc) return chk(rc, "cross q gemm");
      // 6. each lane's own cross-attention
      for (int l = 0; l < nl; ++l)
        if ((rc = cross_core(lanes[l], *Lw[l], N, stream))) return rc;
      // 7. output projection + residual (hB[:, :32]), 8. LayerNorm -> hC (compact)
      GemmProb o[2] = {};
      for (int l = 0; l < nl; ++l) {
        o[l].A = lanes[l].w.ctx16; o[l].a = qc_rows;
        o[l].W = Lw[l]->wco; o[l].bias = Lw[l]->bco;
        o[l].R = lanes[l].w.hB32; o[l].r = q_view;
        o[l].C = lanes[l].w.pre32; o[l].c = qc_rows;
        o[l].M = N * Q; o[l].N = H; o[l].K = H;
      }
      if (ln_fuse && N * Q >= 512) {
        o[0].tile_cfg = GT_RING_96x64;
        o[0].ln_gain = Lw[0]->lncg; o[0].ln_bias = Lw[0]->lncb; o[0].ln_eps = c.ln_eps;
        o[0].ln_y32 = w.hC32; o[0].ln_y32v = qc_rows; o[0].ln_y16 = w.hC16; o[0].ln_y16v = qc_rows; o[0].ln_counter = w.lncnt;
        rc = launch_gemm(o, 1, EPI_RES_LN, op, stream);
        if (rc) return chk(rc, "cross out gemm + ln");
      } else {
        rc = launch_gemm(o, nl, EPI_RES_F32, op, stream);
        if (rc) return chk(rc, "cross out gemm");
        // each lane's compact [N*Q][H] rows start at its own pre32, N*S*H floats apart: one row view with an item per lane
        const RowView pre_v = items_view((long long)N * S * H, N * Q, H), qc_lanes = plain(nl * N * Q, H);
        rc = launch_ln_rows4(w.pre32, pre_v, nl * N * Q, H, Lw[0]->lncg, Lw[0]->lncb, nullptr, nullptr, N * Q, Lw[1]->lncg, Lw[1]->lncb, nullptr, nullptr,
                             1, 1, c.ln_eps, w.hC32, qc_lanes, w.hC16, qc_lanes, op, stream);
        if (rc) return chk(rc, "cross ln");
      }
    }
    // 9-14. feed-forwards: the query problems of every lane, then their text problems (own weights)
    int text_rows = 0;
    RowView tv = t_view;
    if (L > 0) {
      if (!last || want_text_last) text_rows = N * L;
      else if (want_cls_last) { text_rows = N; tv = cls_view; }
    }
    const int ng = text_rows > 0 ? 2 * nl : nl;
    {
      GemmProb g[4] = {};
      for (int l = 0; l < nl; ++l) {
        const Work& v = lanes[l].w;
        GemmProb& q = g[l];
        q.A = cross ? v.hC16 : v.hB16; q.a = fqv;
        q.W = Lw[l]->wiq; q.bias = Lw[l]->biq;
        q.C = v.ffn16; q.c = plain(N * Q, I);
        q.M = N * Q; q.N = I; q.K = H;
        GemmProb& t = g[nl + l];
        t.A = v.hB16 + t_off16; t.a = tv;
        t.W = Lw[l]->wit; t.bias = Lw[l]->bit;
        t.C = v.ffn16 + (size_t)N * Q * I * esz; t.c = plain(text_rows, I);
        t.M = text_rows; t.N = I; t.K = H;
      }
      if ((h->chain_ring & 2) && N * Q >= 512 && I % 192 == 0) g[0].tile_cfg = GT_RING_192x128;
      rc = launch_gemm(g, ng, EPI_GELU_OP, op, stream);
      if (rc) return chk(rc, "ffn up gemm");
    }
    bool ffn_ln_fused = false;
    {
      GemmProb g[4] = {};
      for (int l = 0; l < nl; ++l) {
        const Work& v = lanes[l].w;
        GemmProb& q = g[l];
        q.A = v.ffn16; q.a = plain(N * Q, I);
        q.W = Lw[l]->woq; q.bias = Lw[l]->boq;
        q.R = cross ? v.hC32 : v.hB32; q.r = fqv;
        q.C = v.pre32; q.c = q_view;
        q.M = N * Q; q.N = H; q.K = I;
        GemmProb& t = g[nl + l];
        t.A = v.ffn16 + (size_t)N * Q * I * esz; t.a = plain(text_rows, I);
        t.W = Lw[l]->wot; t.bias = Lw[l]->bot;
        t.R = v.hB32 + t_off32; t.r = tv;
        t.C = v.pre32 + t_off32; t.c = tv;
        t.M = text_rows; t.N = H; t.K = I;
      }
      g[0].tile_cfg = N * Q >= 512 && I % 128 == 0 ? GT_K128_64x128 : GT_AUTO;   // 64 weight rows x 128 activation rows, 128-deep K steps (see the QKV note)
      if ((h->chain_ring & 4) && N * Q >= 512 && H % 96 == 0) g[0].tile_cfg = GT_RING_96x64;
      ffn_ln_fused = ln_fuse && !last && g[0].tile_cfg == GT_RING_96x64;
      if (ffn_ln_fused) {
        // HF:573-587 for both row sets in the same launch: problem 0 = query rows (output_query.LayerNorm), problem 1 = text rows (output.LayerNorm)
        g[0].ln_gain = Lw[0]->lnqg; g[0].ln_bias = Lw[0]->lnqb; g[0].ln_eps = c.ln_eps;
        g[0].ln_y32 = w.hA32; g[0].ln_y32v = q_view; g[0].ln_y16 = w.hA16; g[0].ln_y16v = q_view; g[0].ln_counter = w.lncnt;
        g[1].ln_gain = Lw[0]->lntg; g[1].ln_bias = Lw[0]->lntb; g[1].ln_eps = c.ln_eps;
        g[1].ln_y32 = w.hA32 + t_off32; g[1].ln_y32v = tv; g[1].ln_y16 = w.hA16 + t_off16; g[1].ln_y16v = tv;
        g[1].ln_counter = w.lncnt + (N * Q + 63) / 64;
        rc = launch_gemm(g, ng, EPI_RES_LN, op, stream);
        if (rc) return chk(rc, "ffn down gemm + ln");
      } else {
        rc = launch_gemm(g, ng, EPI_RES_F32, op, stream);
        if (rc) return chk(rc, "ffn down gemm");
      }
    }
    if (ffn_ln_fused) {
      // the LayerNorms ran inside the down-projection's launch
    } else if (!last) {
      // query and text LayerNorms of every lane in one launch over the whole [nl N, S, H] stream
      rc = launch_ln_rows4(w.pre32, all_lanes, nl * N * S, H, Lw[0]->lnqg, Lw[0]->lnqb, Lw[0]->lntg, Lw[0]->lntb, N * S, Lw[1]->lnqg, Lw[1]->lnqb,
                           Lw[1]->lntg, Lw[1]->lntb, S, Q, c.ln_eps, w.hA32, all_lanes, w.hA16, all_lanes, op, stream);
      if (rc) return chk(rc, "ffn ln");
    } else {
      for (int l = 0; l < nl; ++l) {   // last layer: LayerNorm straight into the caller's buffers
        const Lane& x = lanes[l];
        const LayerW& W = *Lw[l];
        if (x.out_full) {
          rc = launch_ln_rows(x.w.pre32, q_view, N * Q, H, W.lnqg, W.lnqb, c.ln_eps, x.out_full, q_view, nullptr, q_view, op, stream);
          if (rc) return chk(rc, "final query ln");
          if (text_rows > 0) {
            rc = launch_ln_rows(x.w.pre32 + t_off32, tv, text_rows, H, W.lntg, W.lntb, c.ln_eps, x.out_full + t_off32, tv, nullptr, tv, op, stream);
            if (rc) return chk(rc, "final text ln");
          }
          if (x.out_query) {
            rc = launch_copy_rows_f32(x.out_full, q_view, x.out_query, qc_rows, N * Q, H, stream);
            if (rc) return chk(rc, "copy out_query");
          }
          if (x.out_cls) {
            rc = launch_copy_rows_f32(x.out_full + t_off32, cls_view, x.out_cls, plain(N, H), N, H, stream);
            if (rc) return chk(rc, "copy out_cls");
          }
        } else {
          if (x.out_query) {
            rc = launch_ln_rows(x.w.pre32, q_view, N * Q, H, W.lnqg, W.lnqb, c.ln_eps, x.out_query, qc_rows, nullptr, qc_rows, op, stream);
            if (rc) return chk(rc, "final query ln");
          }
          if (x.out_cls) {
            rc = launch_ln_rows(x.w.pre32 + t_off32, cls_view, N, H, W.lntg, W.lntb, c.ln_eps, x.out_cls, plain(N, H), nullptr, plain(N, H), op,
                                stream);
            if (rc) return chk(rc, "final cls ln");
          }
        }
      }
    }
  }
  return MRA_OK;
}

// mra_qformer_forward in the precision in force, or (probe) as the probing forward of the automatic precision
int forward_run(mra_qformer* h, bool probe, const int64_t* input_ids, const int64_t* attention_mask, const float* query_embeds,
                int32_t query_items, const void* enc, int32_t items, int32_t L, int32_t kv, float* out_query, float* out_full, float* out_cls,
                void* workspace, size_t workspace_bytes, void* stream_, bool raw = false) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (items < 0 || L < 0 || kv < 0) return fail(MRA_EINVAL, "negative size");
  if (items == 0) return MRA_OK;
  const mra_cfg& c = h->cfg;
  if (kv == 0) return fail(MRA_EINVAL, "kv must be >= 1");
  if (L > c.max_pos) return fail(MRA_EINVAL, "L exceeds max_pos");
  if (!enc || (L > 0 && !input_ids)) return fail(MRA_EINVAL, "null input");
  if (out_cls && L < 1) return fail(MRA_EINVAL, "out_cls needs L >= 1");
  if (query_embeds && query_items != 1 && query_items != items)
    return fail(MRA_EINVAL, "query_items must be 1 or items");
  if (!out_query && !out_full && !out_cls) return fail(MRA_EINVAL, "no output requested");
  if (int rc = check_loaded(h)) return rc;
  Lane lane = make_lane(h, enc, kv, h->cross_precise, probe, raw);
  if (raw && !lane.plan.raw) return fail(MRA_ESTATE, "raw features are not supported in this form: ask mra_qformer_raw_features_ok");
  // the probe needs its own form's workspace; every other forward what mra_qformer_workspace_bytes promises
  const size_t need = probe ? work_bytes(lane, items, L) : mra_qformer_workspace_bytes(h, items, L, kv);
  if (!workspace || workspace_bytes < need)
    return fail(MRA_ENOMEM, "workspace too small: need " + std::to_string(need) + " bytes");
  if (reinterpret_cast<uintptr_t>(workspace) % 256) return fail(MRA_EINVAL, "workspace must be 256-byte aligned");
  if (query_embeds) {
    lane.query = query_embeds;
    lane.query_stride = query_items == items && items > 1 ? (long long)c.n_query * c.hidden : 0;
  }
  lane.out_query = out_query;
  lane.out_full = out_full;
  lane.out_cls = out_cls;
  return run_lanes(&lane, 1, input_ids, attention_mask, items, L, workspace, as_stream(stream_));
}

// Lower median of the p_max histogram of one cross layer, at the centre of its bin (-1 for an empty histogram)
float hist_median(const int* bins) {
  long long n = 0;
  for (int b = 0; b < 256; ++b) n += bins[b];
  if (n == 0) return -1.f;
  long long acc = 0;
  for (int b = 0; b < 256; ++b) {
    acc += bins[b];
    if (2 * acc >= n) return (b + 0.5f) / 256.f;
  }
  return -1.f;
}

// The probing forward of the automatic precision: the op-precision folded chain with the probe kernel, ONE copy of the histograms to pinned
// host memory and ONE synchronisation of the caller's stream, the decision, and -- when it is split, or op in a form other than the probe's --
// the same forward again in the resolved precision, so the caller receives the outputs of the precision in force from here on.
int forward_probe(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask, const float* query_embeds, int32_t query_items,
                  const void* enc, int32_t items, int32_t L, int32_t kv, float* out_query, float* out_full, float* out_cls, void* workspace,
                  size_t workspace_bytes, void* stream_) {
  hipStream_t stream = as_stream(stream_);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(stream, &cap));
  if (cap != hipStreamCaptureStatusNone) return fail(MRA_ESTATE, "auto precision unresolved: run one forward outside capture");
  const size_t hist_bytes = (size_t)h->ncross * 256 * sizeof(int);
  HIP_TRY(hipMemsetAsync(h->auto_hist, 0, hist_bytes, stream));
  h->cross_precise = 0;
  int rc = forward_run(h, true, input_ids, attention_mask, query_embeds, query_items, enc, items, L, kv, out_query, out_full, out_cls, workspace,
                       workspace_bytes, stream_);
  if (rc) return rc;   // the probe stays pending
  HIP_TRY(hipMemcpyAsync(h->auto_hist_host, h->auto_hist, hist_bytes, hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  float worst = 0.f;
  for (int ci = 0; ci < h->ncross; ++ci) {
    h->auto_median[ci] = hist_median(h->auto_hist_host + (size_t)ci * 256);
    worst = std::max(worst, h->auto_median[ci]);
  }
  ++h->auto_probes;
  h->auto_stale = false;
  h->auto_resolved = worst * 1000.f >= (float)h->auto_tau_milli ? 1 : 0;
  h->cross_precise = h->auto_resolved;
  // resolved to op: the probe's outputs are op's own bits when op runs the same form here (the folded form with in-register factors or the
  // rescale pass: same bits); the K/V-cache form (Kv < 2048 in cross mode 0, or mode 1) and the streaming kernels are re-run
  if (h->auto_resolved == 0 && cross_plan(h, kv, false, false).form == CrossPlan::FOLD) return MRA_OK;
  return forward_run(h, false, input_ids, attention_mask, query_embeds, query_items, enc, items, L, kv, out_query, out_full, out_cls, workspace,
                     workspace_bytes, stream_);
}
}  // namespace

int mra_qformer_forward(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask,
                        const float* query_embeds, int32_t query_items, const void* enc, int32_t items, int32_t L,
                        int32_t kv, float* out_query, float* out_full, float* out_cls, void* workspace,
                        size_t workspace_bytes, void* stream_) {
  if (h && h->cross_auto && h->auto_stale && h->ncross > 0 && items > 0)
    return forward_probe(h, input_ids, attention_mask, query_embeds, query_items, enc, items, L, kv, out_query, out_full, out_cls, workspace,
                         workspace_bytes, stream_);
  return forward_run(h, false, input_ids, attention_mask, query_embeds, query_items, enc, items, L, kv, out_query, out_full, out_cls, workspace,
                     workspace_bytes, stream_);
}

// can a forward of h over kv tokens per item read RAW features (x_dtype) in place of mra_modality_ln's output?
static bool raw_ok(mra_qformer* h, int kv, int x_dtype) {
  if (!h || kv <= 0 || h->ncross == 0 || !h->raw_features || x_dtype != h->cfg.op_dtype) return false;
  if (h->cross_precise || (h->cross_auto && (h->auto_stale || h->auto_resolved != 0))) return false;   // split precision; a pending probe
  if (!h->params["ln.weight"].loaded || !h->params["ln.bias"].loaded) return false;
  return cross_plan(h, kv, false, false, true).raw;
}

int mra_qformer_raw_features_ok(mra_qformer* h, int32_t kv, int32_t x_dtype) { return raw_ok(h, kv, x_dtype) ? 1 : 0; }

int mra_qformer_forward_raw(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask, const float* query_embeds,
                            int32_t query_items, const void* enc, int32_t items, int32_t L, int32_t kv, float* out_query, float* out_full,
                            float* out_cls, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (!raw_ok(h, kv, h->cfg.op_dtype)) return fail(MRA_ESTATE, "raw features are not supported in this form: ask mra_qformer_raw_features_ok");
  return forward_run(h, false, input_ids, attention_mask, query_embeds, query_items, enc, items, L, kv, out_query, out_full, out_cls, workspace,
                     workspace_bytes, stream_, true);
}

size_t mra_qformer_pair_workspace_bytes(mra_qformer* h0, mra_qformer* h1, int32_t items, int32_t L, int32_t kv0, int32_t kv1) {
  if (!h0 || !h1 || items <= 0 || L < 0 || kv0 <= 0 || kv1 <= 0) return 0;
  // (a raw-feature lane adds its token factors behind its other buffers: asked for whenever that form could run)
  Lane lanes[2] = {make_lane(h0, nullptr, kv0, h0->cross_precise, false, true), make_lane(h1, nullptr, kv1, h1->cross_precise, false, true)};
  return layout_lanes(lanes, 2, nullptr, items, L);
}

// Pair forward: the layer chains of two Q-Formers of equal shape in ONE launch sequence (run_lanes with two lanes).  raw_mask bit l: lane l's
// encoder features are raw (mra_qformer_forward_raw's form for that lane).
static int forward_pair(mra_qformer* h0, mra_qformer* h1, const int64_t* input_ids, const int64_t* attention_mask, const void* enc0,
                        const void* enc1, int32_t items, int32_t L, int32_t kv0, int32_t kv1, float* out_query0, float* out_cls0,
                        float* out_query1, float* out_cls1, void* workspace, size_t workspace_bytes, void* stream_, int raw_mask) {
  if (!h0 || !h1) return fail(MRA_EINVAL, "null handle");
  if (h0 == h1) return fail(MRA_EINVAL, "the two lanes need two handles");
  if (items < 0 || L < 0 || kv0 < 0 || kv1 < 0) return fail(MRA_EINVAL, "negative size");
  if (items == 0) return MRA_OK;
  mra_qformer* hs[2] = {h0, h1};
  const void* encs[2] = {enc0, enc1};
  const int kvs[2] = {kv0, kv1};
  float* outq[2] = {out_query0, out_query1};
  float* outc[2] = {out_cls0, out_cls1};
  const mra_cfg& c = h0->cfg;
  {
    const mra_cfg& d = h1->cfg;
    if (c.hidden != d.hidden || c.heads != d.heads || c.inter != d.inter || c.layers != d.layers || c.cross_freq != d.cross_freq || c.n_query != d.n_query ||
        c.op_dtype != d.op_dtype || c.ln_eps != d.ln_eps || h0->device != h1->device)
      return fail(MRA_EINVAL, "pair forward: the two Q-Formers must agree in hidden / heads / inter / layers / cross_freq / n_query / op_dtype and live on one device");
  }
  if (kv0 == 0 || kv1 == 0) return fail(MRA_EINVAL, "kv must be >= 1");
  if (L > c.max_pos || L > h1->cfg.max_pos) return fail(MRA_EINVAL, "L exceeds max_pos");
  if (!enc0 || !enc1 || (L > 0 && !input_ids)) return fail(MRA_EINVAL, "null input");
  if ((out_cls0 || out_cls1) && L < 1) return fail(MRA_EINVAL, "out_cls needs L >= 1");
  Lane lanes[2] = {};
  for (int l = 0; l < 2; ++l) {
    if (!outq[l] && !outc[l]) return fail(MRA_EINVAL, "no output requested for a lane");
    if (hs[l]->cross_precise) return fail(MRA_ESTATE, "pair forward runs the operand-dtype score chain: use mra_qformer_forward for split precision");
    if (hs[l]->cross_auto && (hs[l]->auto_stale || hs[l]->auto_resolved != 0))
      return fail(MRA_ESTATE, "pair forward runs the operand-dtype score chain: auto precision must have resolved to op (use mra_qformer_forward)");
    const bool raw = raw_mask >> l & 1;
    if (raw && !raw_ok(hs[l], kvs[l], hs[l]->cfg.op_dtype)) return fail(MRA_ESTATE, "raw features are not supported in this form: ask mra_qformer_raw_features_ok");
    lanes[l] = make_lane(hs[l], encs[l], kvs[l], false, false, raw);
    if (lanes[l].plan.form == CrossPlan::FOLD_STREAM) return fail(MRA_ESTATE, "pair forward: the streaming fold kernels are not supported");
    if (int rc = check_loaded(hs[l])) return rc;
    lanes[l].out_query = outq[l];
    lanes[l].out_cls = outc[l];
  }
  const size_t need = mra_qformer_pair_workspace_bytes(h0, h1, items, L, kv0, kv1);
  if (!workspace || workspace_bytes < need) return fail(MRA_ENOMEM, "workspace too small: need " + std::to_string(need) + " bytes");
  if (reinterpret_cast<uintptr_t>(workspace) % 256) return fail(MRA_EINVAL, "workspace must be 256-byte aligned");
  return run_lanes(lanes, 2, input_ids, attention_mask, items, L, workspace, as_stream(stream_));
}

int mra_qformer_forward_pair(mra_qformer* h0, mra_qformer* h1, const int64_t* input_ids, const int64_t* attention_mask, const void* enc0,
                             const void* enc1, int32_t items, int32_t L, int32_t kv0, int32_t kv1, float* out_query0, float* out_cls0,
                             float* out_query1, float* out_cls1, void* workspace, size_t workspace_bytes, void* stream_) {
  return forward_pair(h0, h1, input_ids, attention_mask, enc0, enc1, items, L, kv0, kv1, out_query0, out_cls0, out_query1, out_cls1, workspace,
                      workspace_bytes, stream_, 0);
}

int mra_qformer_forward_pair_raw(mra_qformer* h0, mra_qformer* h1, const int64_t* input_ids, const int64_t* attention_mask, const void* enc0,
                                 const void* enc1, int32_t raw_mask, int32_t items, int32_t L, int32_t kv0, int32_t kv1, float* out_query0,
                                 float* out_cls0, float* out_query1, float* out_cls1, void* workspace, size_t workspace_bytes, void* stream_) {
  if (raw_mask < 0 || raw_mask > 3) return fail(MRA_EINVAL, "raw_mask has bits 0 and 1");
  return forward_pair(h0, h1, input_ids, attention_mask, enc0, enc1, items, L, kv0, kv1, out_query0, out_cls0, out_query1, out_cls1, workspace,
                      workspace_bytes, stream_, raw_mask);
}

namespace {
// the lane of a multi-prompt forward: always the K/V-cache form in operand precision, `prompts` chain items per encoder item
void make_multi_lane(Lane& x, mra_qformer* h, const void* enc, int kv, int prompts) {
  x = make_lane(h, enc, kv, false, false);
  x.plan.form = CrossPlan::KV_CACHE;
  x.share = prompts;
}
}  // namespace

size_t mra_qformer_multi_workspace_bytes(mra_qformer* h, int32_t enc_items, int32_t prompts, int32_t L, int32_t kv) {
  if (!h || enc_items <= 0 || prompts <= 0 || L < 0 || kv <= 0) return 0;
  if ((long long)enc_items * prompts > 0x7fffffffLL) return 0;
  Lane x;
  make_multi_lane(x, h, nullptr, kv, prompts);
  return layout_lanes(&x, 1, nullptr, enc_items * prompts, L);
}

// Multi-prompt forward: `prompts` chain items per encoder item over ONE K/V projection (run_lanes with a lane whose share count is prompts).
int mra_qformer_forward_multi(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask, const void* enc, int32_t enc_items,
                              int32_t prompts, int32_t L, int32_t kv, float* out_query, float* out_cls, void* workspace, size_t workspace_bytes,
                              void* stream_) {
  if (prompts < 1) return fail(MRA_EINVAL, "prompts must be >= 1");
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (enc_items < 0 || L < 0 || kv < 0) return fail(MRA_EINVAL, "negative size");
  if (enc_items == 0) return MRA_OK;
  if ((long long)enc_items * prompts > 0x7fffffffLL) return fail(MRA_EINVAL, "enc_items * prompts exceeds int32");
  const mra_cfg& c = h->cfg;
  if (kv == 0) return fail(MRA_EINVAL, "kv must be >= 1");
  if (L > c.max_pos) return fail(MRA_EINVAL, "L exceeds max_pos");
  if (!enc || (L > 0 && !input_ids)) return fail(MRA_EINVAL, "null input");
  if (out_cls && L < 1) return fail(MRA_EINVAL, "out_cls needs L >= 1");
  if (!out_query && !out_cls) return fail(MRA_EINVAL, "no output requested");
  if (h->cross_precise) return fail(MRA_ESTATE, "multi forward runs the operand-dtype K/V cache: use mra_qformer_forward for split precision");
  if (h->cross_auto && (h->auto_stale || h->auto_resolved != 0))
    return fail(MRA_ESTATE, "multi forward runs the operand-dtype K/V cache: auto precision must have resolved to op (use mra_qformer_forward)");
  if (int rc = check_loaded(h)) return rc;
  Lane lane;
  make_multi_lane(lane, h, enc, kv, prompts);
  const size_t need = mra_qformer_multi_workspace_bytes(h, enc_items, prompts, L, kv);
  if (!workspace || workspace_bytes < need) return fail(MRA_ENOMEM, "workspace too small: need " + std::to_string(need) + " bytes");
  if (reinterpret_cast<uintptr_t>(workspace) % 256) return fail(MRA_EINVAL, "workspace must be 256-byte aligned");
  lane.out_query = out_query;
  lane.out_cls = out_cls;
  return run_lanes(&lane, 1, input_ids, attention_mask, enc_items * prompts, L, workspace, as_stream(stream_));
}

namespace {
int shared_kv_split(int enc_items, int prompts, int heads, int kv, int core) {
  return core == 1 ? attn_shared_pick_split(enc_items, prompts, heads, kv) : attn_pick_split(enc_items * prompts, heads, 32, kv);
}
}  // namespace

size_t mra_debug_shared_kv_workspace_bytes(int32_t enc_items, int32_t prompts, int32_t heads, int32_t kv, int32_t core) {
  if (enc_items <= 0 || prompts <= 0 || heads <= 0 || kv <= 0 || core < 0 || core > 1) return 0;
  if ((long long)enc_items * prompts > 0x7fffffffLL) return 0;
  return attn_partial_bytes(enc_items * prompts, heads, 32, shared_kv_split(enc_items, prompts, heads, kv, core));
}

// The cross core of the multi forward on its own, through the launch code the forward uses (launch_attention with kv_share, or
// launch_attention_shared), split rule included.
int mra_debug_shared_kv_attention(const void* q, const void* k, const void* v, int32_t dtype, int32_t enc_items, int32_t prompts, int32_t heads,
                                  int32_t kv, int32_t core, void* ctx, void* workspace, size_t workspace_bytes, void* stream) {
  if (enc_items < 0 || prompts < 1 || heads < 1 || kv < 1) return fail(MRA_EINVAL, "sizes: enc_items >= 0, prompts / heads / kv >= 1");
  if (core < 0 || core > 1) return fail(MRA_EINVAL, "core must be 0 (kv_share) or 1 (shared stream)");
  if (dtype != MRA_F16 && dtype != MRA_BF16) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (enc_items == 0) return MRA_OK;
  if (!q || !k || !v || !ctx) return fail(MRA_EINVAL, "null argument");
  if ((long long)enc_items * prompts > 0x7fffffffLL) return fail(MRA_EINVAL, "enc_items * prompts exceeds int32");
  const size_t need = mra_debug_shared_kv_workspace_bytes(enc_items, prompts, heads, kv, core);
  if (need && (!workspace || workspace_bytes < need)) return fail(MRA_ENOMEM, "workspace too small: need " + std::to_string(need) + " bytes");
  if (need && reinterpret_cast<uintptr_t>(workspace) % 16) return fail(MRA_EINVAL, "workspace must be 16-byte aligned");
  AttnArgs a{};
  a.Q = q; a.K = k; a.V = v; a.O = ctx;
  a.q_item_stride = a.o_item_stride = (long long)32 * heads * 64; a.q_ld = a.o_ld = heads * 64;
  a.k_item_stride = a.v_item_stride = (long long)heads * kv * 64; a.k_head_stride = a.v_head_stride = (long long)kv * 64; a.k_ld = a.v_ld = 64;
  a.items = enc_items * prompts; a.heads = heads; a.q_rows = 32; a.kv_len = kv; a.scale = 0.125f;
  a.nsplit = shared_kv_split(enc_items, prompts, heads, kv, core);
  a.part = a.nsplit > 1 ? (float*)workspace : nullptr;
  a.kv_share = prompts;
  const int op = dtype == MRA_BF16 ? OP_BF16 : OP_F16;
  const int rc = core == 1 ? launch_attention_shared(a, op, as_stream(stream)) : launch_attention(a, op, as_stream(stream));
  return rc ? chk(rc, "shared K/V attention") : MRA_OK;
}

// The attention backward core on its own, in the cross-attention layout mra_qformer_backward gives it (compact query-side rows, head-major K/V).
int mra_debug_attention_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse, int32_t dtype,
                            int32_t kv_items, int32_t share, int32_t heads, int32_t q_rows, int32_t kv, void* dq, void* dk, void* dv, void* stream) {
  if (kv_items < 1 || share < 1 || heads < 1 || q_rows < 1 || kv < 1) return fail(MRA_EINVAL, "sizes: kv_items / share / heads / q_rows / kv >= 1");
  if (dtype != MRA_F16 && dtype != MRA_BF16) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (!q || !k || !v || !o || !d_o || !lse || !dq || !dk || !dv) return fail(MRA_EINVAL, "null argument");
  if ((long long)kv_items * share > 0x7fffffffLL) return fail(MRA_EINVAL, "kv_items * share exceeds int32");
  const int limit = attn_bwd_max_share(q_rows);
  if (share > limit)
    return fail(MRA_EINVAL, "share " + std::to_string(share) + " exceeds " + std::to_string(limit) + ", what the backward core's LDS holds at " +
                                std::to_string(q_rows) + " query rows");
  AttnBwdArgs g{};
  g.Q = q; g.K = k; g.V = v; g.O = o; g.dO = d_o; g.dQ = dq; g.dK = dk; g.dV = dv;
  const int H = heads * 64;
  g.q_item_stride = g.o_item_stride = g.dq_item_stride = (long long)q_rows * H; g.q_ld = g.o_ld = g.dq_ld = H;
  g.k_item_stride = g.v_item_stride = g.dk_item_stride = g.dv_item_stride = (long long)heads * kv * 64;
  g.k_head_stride = g.v_head_stride = g.dk_head_stride = g.dv_head_stride = (long long)kv * 64;
  g.k_ld = g.v_ld = g.dk_ld = g.dv_ld = 64;
  g.lse = lse; g.items = kv_items * share; g.heads = heads; g.q_rows = q_rows; g.kv_len = kv; g.scale = 0.125f;
  g.kv_share = share;
  const int rc = launch_attn_bwd(g, dtype == MRA_BF16 ? OP_BF16 : OP_F16, as_stream(stream));
  return rc ? chk(rc, "attention backward") : MRA_OK;
}

int mra_qformer_set_kv_events(mra_qformer* h, void* ev_start, void* ev_stop) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if ((ev_start == nullptr) != (ev_stop == nullptr)) return fail(MRA_EINVAL, "give both events or neither");
  h->kv_ev0 = reinterpret_cast<hipEvent_t>(ev_start);
  h->kv_ev1 = reinterpret_cast<hipEvent_t>(ev_stop);
  return MRA_OK;
}

int mra_qformer_prepare(mra_qformer* h, void* stream) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (h->ncross == 0) return MRA_OK;
  const mra_cfg& c = h->cfg;
  const size_t H = c.hidden, E = c.enc_width, esz = 2;
  if (h->cross_precise && h->precise_stale) {
    // split-precision cross-attention: W_cq as [H][3H] = (hi | hi | lo), W_k as [heads][E][192] = (hi | hi | lo), from the f32 copies
    int ci = 0;
    for (int i = 0; i < c.layers; ++i) {
      if (h->layers[i].cross_index < 0) continue;
      char* base = h->arena_p + (size_t)ci * precise_layer_bytes(h);
      int rc = launch_split_weight(h->layers[i].wcq32, (int)H, (int)H, base, h->op(), as_stream(stream));
      if (!rc) rc = launch_split_key_weight(h->wk32 + (size_t)ci * H * E, c.heads, (int)E, base + precise_wk_off(h), h->op(), as_stream(stream));
      if (rc) return chk(rc, "split-precision weight preparation");
      ++ci;
    }
    h->precise_stale = false;
  }
  if (!h->fold_stale) return MRA_OK;
  for (int ci = 0; ci < h->ncross; ++ci) {   // W_k [H][E] of cross layer ci -> [heads][E][64]
    const int rc = launch_transpose_pad((const char*)h->wkv + (size_t)(ci * 2) * H * E * esz, h->arena_f + (size_t)ci * H * E * esz, 64, (int)E,
                                        64, (long long)64 * E, (long long)E * 64, c.heads, h->op(), as_stream(stream));
    if (rc) return chk(rc, "key weight regroup");
  }
  if (h->params["ln.weight"].loaded && h->params["ln.bias"].loaded) {
    // the raw-feature form's weights: the modality LayerNorm's gain and centring inside W_k and W_v, its bias inside the value bias; from the
    // fp32 copies where the handle keeps them (the key weights), rounded to the operand dtype once
    for (int ci = 0; ci < h->ncross; ++ci) {
      const char* wk = (const char*)h->wkv + (size_t)(ci * 2) * H * E * esz;
      const char* wv = (const char*)h->wkv + (size_t)(ci * 2 + 1) * H * E * esz;
      int rc = h->wk32 ? launch_fold_ln_weight(h->wk32 + (size_t)ci * H * E, 1, (int)H, (int)E, h->encg, h->encb, nullptr, fold_raw_wk(h, ci), 1, nullptr, h->op(), as_stream(stream))
                       : launch_fold_ln_weight(wk, 0, (int)H, (int)E, h->encg, h->encb, nullptr, fold_raw_wk(h, ci), 1, nullptr, h->op(), as_stream(stream));
      if (!rc) rc = launch_fold_ln_weight(wv, 0, (int)H, (int)E, h->encg, h->encb, h->bkv + (size_t)(ci * 2 + 1) * H, fold_raw_wv(h, ci), 0, fold_raw_bv(h, ci), h->op(), as_stream(stream));
      if (rc) return chk(rc, "raw-feature weight preparation");
    }
  }
  h->fold_stale = false;
  return MRA_OK;
}

int mra_qformer_set_cross_mode(mra_qformer* h, int32_t mode) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (mode < 0 || mode > 5)
    return fail(MRA_EINVAL, "cross mode must be 0 (automatic), 1 (K/V cache), 2 (folded), 3 (folded, 128x384 loader-wave tiles), 4 (folded, streaming kernels) or 5 (folded, separate rescale pass)");
  h->cross_mode = mode >= 3 ? 2 : mode;
  h->fold_tile = mode == 3 ? GT_WS_128x384 : GT_128;
  h->fold_stream = mode == 4;     // measured 13 % slower than the loader-wave GEMMs + rescale pass: opt-in
  h->inreg_rescale = mode != 5;   // 5: the round-1 form with a rescale pass over P between the two big GEMMs, kept as the measured alternative
  return MRA_OK;
}

int mra_qformer_set_cross_precision(mra_qformer* h, int32_t mode) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (mode < 0 || mode > 2)
    return fail(MRA_EINVAL, "cross precision must be 0 (operand dtype), 1 (split: hi + lo pairs along the score chain) or 2 (auto: chosen by a probe)");
  if (mode >= 1) {
    const mra_cfg& c = h->cfg;
    if (h->ncross == 0) return fail(MRA_EINVAL, "no cross-attention layers");
    if (!cross_plan(h, 1, true, false).softpart)   // (the form of a split-precision plan does not depend on kv)
      return fail(MRA_EINVAL, "split precision needs heads * n_query == 384 (the 176 x 384 scores tile)");
    if (!h->arena_p || (mode == 2 && !h->auto_hist)) {   // allocations happen on the handle's device
      int dev = 0;
      HIP_TRY(hipGetDevice(&dev));
      if (dev != h->device) return fail(MRA_EINVAL, "handle belongs to another device");
    }
    if (!h->arena_p) {
      const hipError_t e = hipMalloc((void**)&h->arena_p, (size_t)h->ncross * precise_layer_bytes(h));
      if (e != hipSuccess) return fail(MRA_ENOMEM, std::string("split-precision weight arena: ") + hipGetErrorString(e));
      h->precise_stale = true;
    }
    if (mode == 2 && !h->auto_hist) {
      const size_t hist_bytes = (size_t)h->ncross * 256 * sizeof(int);
      hipError_t e = hipMalloc((void**)&h->auto_hist, hist_bytes);
      if (e != hipSuccess) return fail(MRA_ENOMEM, std::string("auto-precision histograms: ") + hipGetErrorString(e));
      e = hipHostMalloc((void**)&h->auto_hist_host, hist_bytes, hipHostMallocDefault);
      if (e != hipSuccess) return fail(MRA_ENOMEM, std::string("auto-precision pinned histograms: ") + hipGetErrorString(e));
      h->auto_median.assign(h->ncross, -1.f);
    }
  }
  h->cross_auto = mode == 2;
  h->auto_stale = true;          // (again) mode 2: the next forward probes
  h->cross_precise = mode == 1;  // auto runs op until a probe resolves it
  return MRA_OK;
}

int mra_qformer_cross_precision_report(mra_qformer* h, int32_t* resolved, int32_t* probes, float* median_pmax, int32_t n_layers) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (median_pmax && n_layers < h->ncross) return fail(MRA_EINVAL, "median_pmax needs one float per cross layer (" + std::to_string(h->ncross) + ")");
  if (resolved) *resolved = h->cross_auto ? (h->auto_stale ? -1 : h->auto_resolved) : h->cross_precise;
  if (probes) *probes = h->auto_probes;
  if (median_pmax)
    for (int ci = 0; ci < h->ncross; ++ci) median_pmax[ci] = ci < (int)h->auto_median.size() ? h->auto_median[ci] : -1.f;
  return MRA_OK;
}

int mra_qformer_set_option(mra_qformer* h, const char* name, int32_t value) {
  if (!h || !name) return fail(MRA_EINVAL, "null argument");
  const std::string key(name);
  if (key == "train_ring") {
    if (value < 0 || value > 7) return fail(MRA_EINVAL, "train_ring is a mask of bits 0-2");
    h->train_ring = value;
    return MRA_OK;
  }
  if (key == "raw_features") {
    if (value < 0 || value > 1) return fail(MRA_EINVAL, "raw_features is 0 or 1");
    h->raw_features = value != 0;
    return MRA_OK;
  }
  if (key == "auto_split_pmax_milli") {
    if (value < 0 || value > 1000) return fail(MRA_EINVAL, "auto_split_pmax_milli is a threshold on p_max in [0, 1000] thousandths");
    h->auto_tau_milli = value;   // applies from the next probe on
    return MRA_OK;
  }
  if (key == "chain_ring") {
    if (value < 0 || value > 15) return fail(MRA_EINVAL, "chain_ring is a mask of bits 0-3");
    h->chain_ring = value;
    return MRA_OK;
  }
  if (key == "cross_fuse") {
    if (value < 0 || (value & ~7))
      return fail(MRA_EINVAL, "cross_fuse is a mask of 1 (query projection and Q' in one launch), 2 (row factors inside the P.enc launch) and 4 (context GEMM on the 64 x 64 tile)");
    h->cross_fuse = value;
    return MRA_OK;
  }
  if (key == "self_fuse") {
    if (value < 0 || value > 1) return fail(MRA_EINVAL, "self_fuse is 0 (QKV GEMM, then the self-attention core) or 1 (both in one launch)");
    h->self_fuse = value;
    return MRA_OK;
  }
  if (key == "multi_core") {
    if (value < 0 || value > 1) return fail(MRA_EINVAL, "multi_core is 0 (attn_kernel with kv_share) or 1 (shared-stream core)");
    h->multi_core = value;   // the workspace size of the multi forward follows it (grid-split partials)
    return MRA_OK;
  }
  return fail(MRA_ENAME, "unknown option: " + key);
}

int mra_qformer_set_kv_done_event(mra_qformer* h, void* ev) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  h->kv_done = reinterpret_cast<hipEvent_t>(ev);
  return MRA_OK;
}

size_t mra_kv_cache_bytes(mra_qformer* h, int32_t items, int32_t kv) {
  if (!h || items <= 0 || kv <= 0) return 0;
  return (size_t)h->ncross * 2 * items * kv * h->cfg.hidden * 2;
}

int mra_kv_project(mra_qformer* h, const void* enc, int32_t items, int32_t kv, void* kv_cache, void* stream) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (items < 0 || kv < 0) return fail(MRA_EINVAL, "negative size");
  if (items == 0 || kv == 0 || h->ncross == 0) return MRA_OK;
  if (!enc || !kv_cache) return fail(MRA_EINVAL, "null argument");
  if ((long long)items * kv > 0x7fffffffLL) return fail(MRA_EINVAL, "items * kv exceeds int32");
  return chk(kv_project(h, enc, items, kv, kv_cache, as_stream(stream)), "kv projection gemm");
}

int mra_llm_proj(mra_qformer* h, const float* z, int32_t rows, void* out, int32_t out_dtype, void* workspace,
                 size_t workspace_bytes, void* stream_) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (rows < 0) return fail(MRA_EINVAL, "negative rows");
  if (rows == 0) return MRA_OK;
  const mra_cfg& c = h->cfg;
  if (c.llm_hidden <= 0 || !h->params["llm_proj.weight"].loaded || !h->params["llm_proj.bias"].loaded)
    return fail(MRA_ESTATE, "llm_proj not loaded");
  if (!z || !out || !workspace) return fail(MRA_EINVAL, "null argument");
  const size_t need = align_up((size_t)rows * c.hidden * 2);
  if (workspace_bytes < need) return fail(MRA_ENOMEM, "workspace too small: need " + std::to_string(need));
  const int op = h->op();
  if (out_dtype != MRA_F32 && out_dtype != c.op_dtype) return fail(MRA_EINVAL, "out_dtype must be f32 or the operand dtype");
  hipStream_t stream = as_stream(stream_);
  int rc = launch_convert(z, MRA_F32, workspace, c.op_dtype, (long long)rows * c.hidden, stream);
  if (rc) return chk(rc, "convert z");
  GemmProb p{};
  p.A = workspace; p.a = plain(rows, c.hidden);
  p.W = h->wllm; p.bias = h->bllm;
  p.C = out; p.c = plain(rows, c.llm_hidden);
  p.M = rows; p.N = c.llm_hidden; p.K = c.hidden;
  return chk(launch_gemm(&p, 1, out_dtype == MRA_F32 ? EPI_F32 : EPI_OP, op, stream), "llm_proj gemm");
}

int mra_cosine_score(const float* z, const float* t, int32_t t_rows, int32_t items, int32_t n_query, int32_t hidden,
                     float* sim, float* logit, void* stream) {
  if (items < 0) return fail(MRA_EINVAL, "negative items");
  if (items == 0) return MRA_OK;
  if (!z || !t || !logit) return fail(MRA_EINVAL, "null argument");
  return chk(launch_cosine_score(z, t, t_rows, items, n_query, hidden, 1e-8f, sim, logit, as_stream(stream)), "cosine_score");
}

int mra_fuse_logits(const float* const* logits, const float* weights, int32_t nmod, int32_t n, float* out, void* stream) {
  if (n < 0) return fail(MRA_EINVAL, "negative n");
  if (!logits || !out) return fail(MRA_EINVAL, "null argument");
  for (int m = 0; m < nmod && m < 4; ++m)
    if (!logits[m]) return fail(MRA_EINVAL, "null logits pointer");
  return chk(launch_fuse_logits(logits, weights, nmod, n, out, as_stream(stream)), "fuse_logits");
}

int mra_span_from_logits(const float* logits, int32_t videos, int32_t clips, float alpha, int32_t* spans, void* stream) {
  if (videos < 0) return fail(MRA_EINVAL, "negative videos");
  if (videos == 0) return MRA_OK;
  if (!logits || !spans) return fail(MRA_EINVAL, "null argument");
  return chk(launch_span(logits, videos, clips, alpha, spans, as_stream(stream)), "span_from_logits");
}

int mra_windows_from_logits(const float* logits, int32_t videos, int32_t clips, float alpha, int32_t top_k, float nms_thd,
                            int32_t max_len, int32_t* windows, float* scores, int32_t* counts, void* stream) {
  if (videos < 0) return fail(MRA_EINVAL, "negative videos");
  if (videos == 0) return MRA_OK;
  if (!logits || !windows || !scores || !counts) return fail(MRA_EINVAL, "null argument");
  if (clips < 1 || clips > 4096) return fail(MRA_EINVAL, "clips must be in 1..4096");
  if (top_k < 1 || top_k > 64) return fail(MRA_EINVAL, "top_k must be in 1..64");
  if (!(nms_thd >= 0.f && nms_thd < 1.f)) return fail(MRA_EINVAL, "nms_thd must be in [0, 1)");
  if (max_len < 0) return fail(MRA_EINVAL, "negative max_len (0 = no length cap)");
  return chk(launch_windows(logits, videos, clips, alpha, top_k, nms_thd, max_len, windows, scores, counts, as_stream(stream)),
             "windows_from_logits");
}

// ---- the Q-Former forward's own kernels, one launch each (include/mra.h; tests/test_gpu_qformer_kernels.py) ----------------------------
// Every entry checks its arguments before any launch, allocates nothing and calls the launch function the forward calls.
namespace {
bool dbg_op(int32_t dtype, int* op) {
  if (dtype != MRA_F16 && dtype != MRA_BF16) return false;
  *op = dtype == MRA_BF16 ? OP_BF16 : OP_F16;
  return true;
}
bool dbg_aligned(const void* p, size_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
// a host triple (item_stride, rows per item, row stride) -> RowView; rows of 16-byte multiples
bool dbg_view(const int64_t* v, RowView* out) {
  if (!v || v[1] <= 0 || v[1] > 0x7fffffffLL || v[2] <= 0 || v[2] > 0x7fffffffLL || v[0] < 0 || (v[0] & 3) || (v[2] & 3)) return false;
  *out = RowView{(long long)v[0], (int)v[1], (int)v[2]};
  return true;
}
}  // namespace

int mra_debug_self_attention(const void* qkv, const int64_t* mask, int32_t dtype, int32_t items, int32_t S, int32_t heads, void* ctx, float* lse,
                             void* stream) {
  int op;
  if (items < 0 || S < 1 || heads < 1 || heads > 16) return fail(MRA_EINVAL, "sizes: items >= 0, S >= 1, heads in 1..16");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (items == 0) return MRA_OK;
  if (!qkv || !ctx) return fail(MRA_EINVAL, "null argument");
  if (!dbg_aligned(qkv, 16) || !dbg_aligned(ctx, 16)) return fail(MRA_EINVAL, "qkv and ctx must be 16-byte aligned");
  if ((long long)items * heads * ((S + 31) / 32) > 0x7fffffffLL / 4) return fail(MRA_EINVAL, "items * heads * query blocks exceeds int32");
  mra_cfg c{};
  c.hidden = heads * 64;
  c.heads = heads;
  return chk(launch_attention(self_attn_args(c, qkv, ctx, (const long long*)mask, items, S, lse), op, as_stream(stream)), "self attention");
}

// The attention backward core in the self-attention layout of mra_qformer_backward(_multi): the step's own argument builder for hidden = heads * 64.
int mra_debug_self_attention_bwd(const void* qkv, const int64_t* mask, const void* ctx, const void* d_ctx, const float* lse, int32_t dtype,
                                 int32_t items, int32_t S, int32_t heads, void* dqkv, void* stream) {
  int op;
  if (items < 1 || S < 1 || heads < 1) return fail(MRA_EINVAL, "sizes: items / S / heads >= 1");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (!qkv || !ctx || !d_ctx || !lse || !dqkv) return fail(MRA_EINVAL, "null argument");
  if (!dbg_aligned(qkv, 16) || !dbg_aligned(ctx, 16) || !dbg_aligned(d_ctx, 16) || !dbg_aligned(dqkv, 16))
    return fail(MRA_EINVAL, "qkv, ctx, d_ctx and dqkv must be 16-byte aligned");
  if ((long long)items * heads > 0x7fffffffLL || (long long)heads * 192 > 0x7fffffffLL) return fail(MRA_EINVAL, "items * heads exceeds int32");
  if (attn_bwd_max_share(S) < 1)
    return fail(MRA_EINVAL, "S " + std::to_string(S) + " exceeds 448, what the backward core's LDS holds: ceil(S / 32) <= 14 query blocks");
  mra_cfg c{};
  c.hidden = heads * 64;
  c.heads = heads;
  const int rc = launch_attn_bwd(self_attn_bwd_args(c, qkv, ctx, d_ctx, (const long long*)mask, lse, items, S, dqkv), op, as_stream(stream));
  return rc ? chk(rc, "self attention backward") : MRA_OK;
}

int mra_debug_ln_rows(const float* x, const int64_t* x_view, int32_t rows, int32_t H, const float* const* params, int32_t lane_rows, int32_t period,
                      int32_t split, float eps, float* y32, const int64_t* y32_view, void* y16, const int64_t* y16_view, int32_t dtype, void* stream) {
  int op;
  if (rows < 0) return fail(MRA_EINVAL, "negative rows");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (H <= 0 || H % 256 || H > 1024) return fail(MRA_EINVAL, "H must be a multiple of 256, <= 1024");
  if (period <= 0 || split < 0 || lane_rows < 0) return fail(MRA_EINVAL, "period > 0, split >= 0, lane_rows >= 0");
  if (rows == 0) return MRA_OK;
  if (!x || !params || (!y32 && !y16)) return fail(MRA_EINVAL, "null argument");
  RowView xv{}, y32v{0, 1, H}, y16v{0, 1, H};
  if (!dbg_view(x_view, &xv) || (y32 && !dbg_view(y32_view, &y32v)) || (y16 && !dbg_view(y16_view, &y16v)))
    return fail(MRA_EINVAL, "a row view is (item_stride >= 0, rows per item > 0, row stride > 0), strides multiples of 4");
  if (xv.ld < H || y32v.ld < H || y16v.ld < H) return fail(MRA_EINVAL, "row stride below H");
  if (!dbg_aligned(x, 16) || !dbg_aligned(y32, 16) || !dbg_aligned(y16, 8)) return fail(MRA_EINVAL, "misaligned buffer");
  for (int s = 0; s < 4; ++s)
    if ((params[2 * s] == nullptr) != (params[2 * s + 1] == nullptr)) return fail(MRA_EINVAL, "a parameter set is a (gain, bias) pair");
  if (!params[0]) return fail(MRA_EINVAL, "parameter set 1 is required");
  if (lane_rows < rows && !params[4]) return fail(MRA_EINVAL, "rows from lane_rows on need parameter set 3");
  for (int s = 0; s < 8; ++s)
    if (!dbg_aligned(params[s], 16)) return fail(MRA_EINVAL, "misaligned parameter");
  return chk(launch_ln_rows4(x, xv, rows, H, params[0], params[1], params[2], params[3], lane_rows, params[4], params[5], params[6], params[7], period,
                             split, eps, y32, y32v, y16, y16v, op, as_stream(stream)),
             "ln_rows");
}

int mra_debug_embed_ln(const int64_t* ids, int32_t items, int32_t L, int32_t Q, int32_t H, int32_t vocab, const float* query, int64_t query_item_stride,
                       const float* word, const float* pos, const float* gain, const float* bias, float eps, float* h32, void* h16, float* pre32,
                       int32_t dtype, void* stream) {
  int op;
  if (items < 0 || L < 0 || Q < 0 || vocab < 1) return fail(MRA_EINVAL, "sizes: items, L, Q >= 0, vocab >= 1");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (H <= 0 || H % 256 || H > 1024) return fail(MRA_EINVAL, "H must be a multiple of 256, <= 1024");
  if (query_item_stride < 0 || (query_item_stride & 3)) return fail(MRA_EINVAL, "query_item_stride must be 0 or a multiple of 4");
  if (items == 0 || Q + L == 0) return MRA_OK;
  if (!gain || !bias || !h32 || !h16 || (Q > 0 && !query) || (L > 0 && (!ids || !word || !pos))) return fail(MRA_EINVAL, "null argument");
  if (!dbg_aligned(query, 16) || !dbg_aligned(word, 16) || !dbg_aligned(pos, 16) || !dbg_aligned(gain, 16) || !dbg_aligned(bias, 16) ||
      !dbg_aligned(h32, 16) || !dbg_aligned(h16, 8) || !dbg_aligned(pre32, 16))
    return fail(MRA_EINVAL, "misaligned buffer");
  return chk(launch_embed_ln((const long long*)ids, items, L, Q, H, vocab, query, query_item_stride, word, pos, gain, bias, eps, h32, h16, pre32, op,
                             as_stream(stream)),
             "embed_ln");
}

int mra_debug_modality_ln(const void* x, int32_t x_dtype, const int64_t* item_index, int32_t items, int32_t tokens, int32_t E, const float* gain,
                          const float* bias, float eps, void* out, int32_t dtype, void* stream) {
  int op;
  if (items < 0 || tokens < 0) return fail(MRA_EINVAL, "negative size");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (x_dtype != MRA_F32 && x_dtype != MRA_F16 && x_dtype != MRA_BF16) return fail(MRA_EINVAL, "x_dtype must be f32, f16 or bf16");
  if (E <= 0 || E % 8 || E > 4096) return fail(MRA_EINVAL, "E must be a multiple of 8, <= 4096");
  if (items == 0 || tokens == 0) return MRA_OK;
  if (!x || !gain || !bias || !out) return fail(MRA_EINVAL, "null argument");
  if (!dbg_aligned(x, 16) || !dbg_aligned(gain, 16) || !dbg_aligned(bias, 16) || !dbg_aligned(out, 16)) return fail(MRA_EINVAL, "misaligned buffer");
  return chk(launch_modality_ln(x, x_dtype, (const long long*)item_index, items, tokens, E, gain, bias, eps, out, op, as_stream(stream)), "modality_ln");
}

int mra_debug_softmax_rows(const float* S, int64_t ld_s, void* P, int64_t ld_p, int32_t rows, int32_t kv, int32_t kvp, float scale, int32_t dtype,
                           void* stream) {
  int op;
  if (rows < 0) return fail(MRA_EINVAL, "negative rows");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (kv <= 0 || kvp < kv || (kvp & 3) || ld_s < kv || ld_p < kvp || (ld_s & 3) || (ld_p & 3))
    return fail(MRA_EINVAL, "need 0 < kv <= kvp <= ld_p, kv <= ld_s, and kvp, ld_s, ld_p multiples of 4");
  if (rows == 0) return MRA_OK;
  if (!S || !P) return fail(MRA_EINVAL, "null argument");
  if (!dbg_aligned(S, 16) || !dbg_aligned(P, 8)) return fail(MRA_EINVAL, "misaligned buffer");
  return chk(launch_softmax_rows(S, ld_s, P, ld_p, rows, kv, kvp, scale, op, as_stream(stream)), "softmax_rows");
}

int mra_debug_fold_rowfactor(const float* stat_m, const float* stat_l, float* factors, int32_t rows, int32_t R, int32_t ntiles, void* P, int64_t ld_p,
                             int32_t tile_cols, int32_t kvp, int32_t* hist, void* stream) {
  if (rows < 0) return fail(MRA_EINVAL, "negative rows");
  if (ntiles <= 0 || tile_cols <= 0 || R <= 0 || R > 512 || rows % R) return fail(MRA_EINVAL, "need ntiles, tile_cols > 0, 0 < R <= 512, rows % R == 0");
  if ((long long)ntiles * tile_cols > kvp || ld_p < kvp) return fail(MRA_EINVAL, "need ntiles * tile_cols <= kvp <= ld_p");
  if (rows == 0) return MRA_OK;
  if (!stat_m || !stat_l || !factors || !P) return fail(MRA_EINVAL, "null argument");
  return chk(launch_fold_rowfactor(stat_m, stat_l, factors, rows, R, ntiles, P, ld_p, tile_cols, kvp, as_stream(stream), hist), "fold_rowfactor");
}

int mra_debug_softmax_rescale(void* P, int64_t ld_p, const float* stat_m, const float* stat_l, int32_t rows, int32_t ntiles, int32_t tile_cols,
                              int32_t kvp, int32_t dtype, int32_t* hist, void* stream) {
  int op;
  if (rows < 0) return fail(MRA_EINVAL, "negative rows");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (ntiles <= 0 || ntiles > 128 || tile_cols <= 0 || (tile_cols & 7) || kvp <= 0 || (kvp & 7) || (ld_p & 7) || ld_p < kvp)
    return fail(MRA_EINVAL, "need 0 < ntiles <= 128, and tile_cols, kvp, ld_p positive multiples of 8 with kvp <= ld_p");
  if (rows == 0) return MRA_OK;
  if (!P || !stat_m || !stat_l) return fail(MRA_EINVAL, "null argument");
  if (!dbg_aligned(P, 16)) return fail(MRA_EINVAL, "misaligned buffer");
  return chk(launch_softmax_rescale(P, ld_p, stat_m, stat_l, rows, ntiles, tile_cols, kvp, op, as_stream(stream), hist), "softmax_rescale");
}

int mra_debug_transpose_pad(const void* src, void* dst, int32_t R, int32_t C, int32_t ld_d, int64_t src_bs, int64_t dst_bs, int32_t batch, int32_t dtype,
                            void* stream) {
  int op;
  if (batch < 0 || R < 0 || C < 0) return fail(MRA_EINVAL, "negative size");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (ld_d < R || batch > 65535) return fail(MRA_EINVAL, "need R <= ld_d and batch <= 65535");
  if (batch == 0 || R == 0 || C == 0) return MRA_OK;
  if (!src || !dst) return fail(MRA_EINVAL, "null argument");
  if (src_bs < (long long)R * C || dst_bs < (long long)C * ld_d) return fail(MRA_EINVAL, "batch stride smaller than the matrix");
  // launch_transpose_pad takes its 64 x 64 kernel (16-byte accesses) from C and ld_d alone: the forward's strides and buffers always fit it
  if (C % 8 == 0 && ld_d % 8 == 0 && C >= 64 && ld_d >= 64 && (src_bs % 8 || dst_bs % 8 || !dbg_aligned(src, 16) || !dbg_aligned(dst, 16)))
    return fail(MRA_EINVAL, "C, ld_d multiples of 8 and >= 64 need 16-byte aligned buffers and batch strides that are multiples of 8");
  return chk(launch_transpose_pad(src, dst, R, C, ld_d, src_bs, dst_bs, batch, op, as_stream(stream)), "transpose_pad");
}

int mra_debug_split(int32_t kind, const float* src, const int64_t* src_view, int32_t rows, int32_t C, int32_t chunk, int32_t parts, void* dst,
                    int32_t dtype, void* stream) {
  int op;
  if (kind < 0 || kind > 2) return fail(MRA_EINVAL, "kind must be 0 (rows), 1 (weight) or 2 (key weight)");
  if (rows < 0 || C <= 0) return fail(MRA_EINVAL, "sizes: rows >= 0, C > 0");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  RowView sv{0, 1, C};
  if (kind == 0) {
    if (chunk <= 0 || C % chunk || chunk % 4 || (parts != 2 && parts != 3)) return fail(MRA_EINVAL, "need chunk % 4 == 0, C % chunk == 0, parts 2 or 3");
    if (!dbg_view(src_view, &sv) || sv.ld < C) return fail(MRA_EINVAL, "bad row view");
  }
  if (rows == 0) return MRA_OK;
  if (!src || !dst) return fail(MRA_EINVAL, "null argument");
  if (!dbg_aligned(src, 16) || !dbg_aligned(dst, 8)) return fail(MRA_EINVAL, "misaligned buffer");
  hipStream_t st = as_stream(stream);
  if (kind == 0) return chk(launch_split_rows(src, sv, rows, C, chunk, parts, dst, op, st), "split_rows");
  if (kind == 1) return chk(launch_split_weight(src, rows, C, dst, op, st), "split_weight");
  return chk(launch_split_key_weight(src, rows, C, dst, op, st), "split_key_weight");
}

// ---- the Q-Former training step's own kernels, one launch each (include/mra.h; tests/test_gpu_train_kernels.py) -------------------------
// As above: every argument is checked before any launch, nothing is allocated, and the launch function is the one mra_train.hip calls.
namespace {
// a row view of 16-bit operand rows read or written in 16-byte pieces: strides multiples of 8 elements
bool dbg_view8(const int64_t* v, RowView* out) { return dbg_view(v, out) && !(v[0] & 7) && !(v[2] & 7); }
constexpr int DBG_TR_MAX_JOBS = 64;
}  // namespace

int mra_debug_gemm_tn_group(int32_t njobs, const void* const* dY, const int64_t* y_views, const int64_t* y_block_stride, const void* const* X,
                            const int64_t* x_views, const int64_t* x_block_stride, float* const* dW, float* const* db, const int32_t* M,
                            const int32_t* N, const int32_t* K, const int32_t* ldw, const int32_t* accumulate, int32_t dtype, void* stream) {
  int op;
  if (njobs < 1 || njobs > GEMM_TN_MAX_JOBS) return fail(MRA_EINVAL, "njobs must be 1 .. 4");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (!dY || !y_views || !y_block_stride || !X || !x_views || !x_block_stride || !dW || !M || !N || !K || !ldw || !accumulate)
    return fail(MRA_EINVAL, "null argument array");
  GemmTnArgs jobs[GEMM_TN_MAX_JOBS];
  for (int i = 0; i < njobs; ++i) {
    GemmTnArgs& a = jobs[i];
    a = GemmTnArgs{};
    if (!dY[i] || !X[i] || !dW[i]) return fail(MRA_EINVAL, "null dY, X or dW");
    if (!dbg_aligned(dY[i], 16) || !dbg_aligned(X[i], 16) || !dbg_aligned(dW[i], 4) || (db && !dbg_aligned(db[i], 4)))
      return fail(MRA_EINVAL, "dY and X must be 16-byte aligned (dW, db: 4)");
    if (M[i] <= 0 || N[i] <= 0 || K[i] <= 0 || N[i] % 64 || K[i] % 64) return fail(MRA_EINVAL, "need M > 0 and N, K positive multiples of 64");
    if (!dbg_view8(y_views + 3 * i, &a.yv) || !dbg_view8(x_views + 3 * i, &a.xv))
      return fail(MRA_EINVAL, "a row view is (item_stride >= 0, rows per item > 0, row stride > 0), strides multiples of 8");
    if (y_block_stride[i] < 0 || x_block_stride[i] < 0 || (y_block_stride[i] & 7) || (x_block_stride[i] & 7))
      return fail(MRA_EINVAL, "block strides must be non-negative multiples of 8");
    if (ldw[i] < K[i]) return fail(MRA_EINVAL, "ldw below K");
    a.dY = dY[i]; a.X = X[i]; a.dW = dW[i]; a.db = db ? db[i] : nullptr;
    a.y_block_stride = y_block_stride[i]; a.x_block_stride = x_block_stride[i];
    a.M = M[i]; a.N = N[i]; a.K = K[i]; a.ldw = ldw[i]; a.accumulate = accumulate[i] ? 1 : 0;
  }
  const int rc = launch_gemm_tn_group(jobs, njobs, op, as_stream(stream));
  // everything else the launchers refuse was refused above: what is left is the group's rule on the split contraction
  if (rc == -1) return fail(MRA_EINVAL, "a group whose contraction is split needs every job accumulating");
  return chk(rc, "gemm_tn group");
}

namespace {
// ptrs: dy, x, gamma, dx, add, dx16, dgamma, dbeta; views: dy, x, dx, add, dx16 (3 each)
const char* dbg_ln_bwd_job(const void* const* p, const int64_t* v, int32_t rows, float eps, int H, LnBwdArgs* out) {
  LnBwdArgs& a = *out;
  a = LnBwdArgs{};
  a.rows = rows;
  a.eps = eps;
  if (!p) return rows > 0 ? "null argument" : nullptr;
  if ((p[6] == nullptr) != (p[7] == nullptr)) return "dgamma and dbeta come as a pair";
  a.dgamma = (float*)p[6];
  a.dbeta = (float*)p[7];
  if (rows == 0) return nullptr;
  if (!v || !p[0] || !p[1] || !p[2] || !p[3]) return "null argument";
  if (!dbg_view(v, &a.dyv) || !dbg_view(v + 3, &a.xv) || !dbg_view(v + 6, &a.dxv) || (p[4] && !dbg_view(v + 9, &a.addv)))
    return "a row view is (item_stride >= 0, rows per item > 0, row stride > 0), strides multiples of 4";
  if (p[5] && !dbg_view8(v + 12, &a.dx16v)) return "the dx16 view needs strides that are multiples of 8";
  if (a.dyv.ld < H || a.xv.ld < H || a.dxv.ld < H || (p[4] && a.addv.ld < H) || (p[5] && a.dx16v.ld < H)) return "row stride below H";
  for (int i = 0; i < 8; ++i)
    if (!dbg_aligned(p[i], 16)) return "misaligned buffer";
  a.dy = (const float*)p[0]; a.x = (const float*)p[1]; a.gamma = (const float*)p[2]; a.dx = (float*)p[3];
  a.add = (const float*)p[4]; a.dx16 = (void*)p[5];
  return nullptr;
}
}  // namespace

int mra_debug_ln_bwd(const void* const* ptrs_a, const int64_t* views_a, int32_t rows_a, float eps_a, const void* const* ptrs_b, const int64_t* views_b,
                     int32_t rows_b, float eps_b, int32_t H, int32_t dtype, void* stream) {
  int op;
  if (rows_a < 0 || rows_b < 0) return fail(MRA_EINVAL, "negative rows");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (H != 256 && H != 512 && H != 768 && H != 1024) return fail(MRA_EINVAL, "H must be 256, 512, 768 or 1024");
  if (!ptrs_b && rows_b > 0) return fail(MRA_EINVAL, "rows_b > 0 without job b");
  LnBwdArgs a, b;
  if (const char* e = dbg_ln_bwd_job(ptrs_a, views_a, rows_a, eps_a, H, &a)) return fail(MRA_EINVAL, std::string("job a: ") + e);
  if (const char* e = dbg_ln_bwd_job(ptrs_b, views_b, rows_b, eps_b, H, &b)) return fail(MRA_EINVAL, std::string("job b: ") + e);
  if (ptrs_a && ptrs_b && (a.dgamma != nullptr) != (b.dgamma != nullptr)) return fail(MRA_EINVAL, "both jobs or neither take dgamma / dbeta");
  return chk(launch_ln_bwd2(a, ptrs_b ? &b : nullptr, H, op, as_stream(stream)), "ln_bwd");
}

int mra_debug_embed_bwd(const float* demb, const int64_t* ids, int32_t items, int32_t L, int32_t Q, int32_t H, int32_t vocab, float* dquery, float* dpos,
                        float* dword, void* stream) {
  if (items < 0) return fail(MRA_EINVAL, "negative items");
  if (H <= 0 || H % 4) return fail(MRA_EINVAL, "H must be a positive multiple of 4");
  if (Q < 0 || L < 0 || Q + (int64_t)L == 0 || Q + (int64_t)L > 0x7fffffffLL) return fail(MRA_EINVAL, "need Q >= 0, L >= 0 and Q + L > 0");
  if (vocab < 1) return fail(MRA_EINVAL, "vocab must be at least 1");
  if (items == 0) return MRA_OK;
  if (!demb) return fail(MRA_EINVAL, "null argument");
  if (L > 0 && dword && !ids) return fail(MRA_EINVAL, "dword needs ids");
  if (!dbg_aligned(demb, 4) || !dbg_aligned(dquery, 4) || !dbg_aligned(dpos, 4) || !dbg_aligned(dword, 4) || !dbg_aligned(ids, 8))
    return fail(MRA_EINVAL, "misaligned buffer");
  return chk(launch_embed_bwd(demb, (const long long*)ids, items, L, Q, H, vocab, dquery, dpos, dword, as_stream(stream)), "embed_bwd");
}

size_t mra_debug_transpose16_batch_scratch_bytes(int32_t njobs) { return njobs < 1 || njobs > DBG_TR_MAX_JOBS ? 0 : (size_t)njobs * sizeof(TrJob); }

int mra_debug_transpose16_batch(const void* const* src, void* const* dst, const int32_t* R, const int32_t* C, int32_t njobs, int32_t dtype, void* scratch,
                                size_t scratch_bytes, void* stream) {
  int op;
  if (njobs < 1 || njobs > DBG_TR_MAX_JOBS) return fail(MRA_EINVAL, "njobs must be 1 .. 64");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (!src || !dst || !R || !C || !scratch) return fail(MRA_EINVAL, "null argument");
  if (scratch_bytes < mra_debug_transpose16_batch_scratch_bytes(njobs) || !dbg_aligned(scratch, 8))
    return fail(MRA_EINVAL, "scratch smaller than mra_debug_transpose16_batch_scratch_bytes, or not 8-byte aligned");
  TrJob jobs[DBG_TR_MAX_JOBS];
  long long tiles = 0;
  for (int i = 0; i < njobs; ++i) {   // the table as refresh_transposes (mra_train.hip) builds it
    if (!src[i] || !dst[i]) return fail(MRA_EINVAL, "null matrix");
    if (R[i] < 1 || C[i] < 1) return fail(MRA_EINVAL, "R and C must be at least 1");
    if (!dbg_aligned(src[i], 2) || !dbg_aligned(dst[i], 2)) return fail(MRA_EINVAL, "misaligned matrix");
    const int tx = (C[i] + 31) / 32, ty = (R[i] + 31) / 32;
    jobs[i] = TrJob{src[i], dst[i], R[i], C[i], (int)tiles, tx};
    tiles += (long long)tx * ty;
    if (tiles > 0x7fffffffLL) return fail(MRA_EINVAL, "too many tiles");
  }
  HIP_TRY(hipMemcpy(scratch, jobs, (size_t)njobs * sizeof(TrJob), hipMemcpyHostToDevice));
  return chk(launch_transpose16_batch((const TrJob*)scratch, njobs, (int)tiles, op, as_stream(stream)), "transpose16_batch");
}

int mra_debug_gemm_gelu(int32_t nprob, const void* const* A, const int64_t* a_views, const void* const* W, const float* const* bias, void* const* C,
                        const int64_t* c_views, void* const* aux, const int32_t* M, const int32_t* N, const int32_t* K, int32_t backward, int32_t tile_cfg,
                        int32_t dtype, void* stream) {
  int op;
  if (nprob < 1 || nprob > 2) return fail(MRA_EINVAL, "one or two problems");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (tile_cfg != GT_AUTO && tile_cfg != GT_64 && tile_cfg != GT_128 && tile_cfg != GT_256) return fail(MRA_EINVAL, "tile_cfg must be GT_AUTO, GT_64, GT_128 or GT_256");
  if (!A || !a_views || !W || !C || !c_views || !aux || !M || !N || !K) return fail(MRA_EINVAL, "null argument array");
  GemmProb ps[2];
  for (int i = 0; i < nprob; ++i) {
    GemmProb& p = ps[i];
    p = GemmProb{};
    if (!A[i] || !W[i] || !C[i] || !aux[i]) return fail(MRA_EINVAL, "null A, W, C or aux");
    if (!dbg_view8(a_views + 3 * i, &p.a)) return fail(MRA_EINVAL, "the A view needs rows per item > 0 and strides that are multiples of 8");
    if (!dbg_view(c_views + 3 * i, &p.c)) return fail(MRA_EINVAL, "the C view needs rows per item > 0 and strides that are multiples of 4");
    if (!dbg_aligned(A[i], 16) || !dbg_aligned(W[i], 16) || !dbg_aligned(C[i], 8) || !dbg_aligned(aux[i], 8) || (bias && !dbg_aligned(bias[i], 16)))
      return fail(MRA_EINVAL, "misaligned buffer");
    p.A = A[i]; p.W = W[i]; p.bias = bias ? bias[i] : nullptr; p.C = C[i]; p.aux = aux[i];
    p.M = M[i]; p.N = N[i]; p.K = K[i];
    if (p.M > 0 && (p.a.ld < p.K || p.c.ld < p.N)) return fail(MRA_EINVAL, "row stride below the row length");
  }
  ps[0].tile_cfg = tile_cfg;   // the first problem decides (Ctx::gemm2)
  const int epi = backward ? EPI_GELU_BWD : EPI_GELU_BOTH;
  GemmPlan pl;
  pl.cus = 0;
  const int rc = gemm_plan(ps, nprob, epi, op, &pl);
  if (rc) return fail(MRA_EINVAL, rc == -2 ? "the tile has no such epilogue" : "gemm_plan refuses the problem (M, N > 0, K % 64, N % tile)");
  return chk(launch_gemm(ps, nprob, epi, op, as_stream(stream)), "gemm gelu");
}

// ---- the forward GEMMs, one launch each (include/mra.h; tests/test_gpu_gemm_forward.py) ----------------------------------------------------
namespace {
typedef unsigned __int128 u128;   // footprints are products of caller-given 63-bit strides and 31-bit counts

// elements from the view's base to one past column cols - 1 of the farthest of its first `rows` rows
u128 dbg_extent(const RowView& v, long long rows, long long cols) {
  if (rows <= 0 || cols <= 0) return 0;
  const long long last_item = (rows - 1) / v.rpi, last_row = (rows - 1) % v.rpi;
  u128 far = (u128)last_item * (u128)v.item_stride + (u128)last_row * (u128)v.ld;
  if (last_item > 0) {   // a full item before the last one may reach further (item stride below rpi * ld)
    const u128 full = (u128)(last_item - 1) * (u128)v.item_stride + (u128)(v.rpi - 1) * (u128)v.ld;
    if (full > far) far = full;
  }
  return far + (u128)cols;
}
bool dbg_fits(u128 elements, size_t esz, u128 extra_bytes, uint64_t have) { return elements * esz + extra_bytes <= (u128)have; }

// the descriptor -> GemmProb, everything that needs no tile checked; nullptr or the reason for a refusal
const char* dbg_gemm_prob(const mra_gemm_desc& d, int epi, GemmProb* out) {
  GemmProb& p = *out;
  p = GemmProb{};
  if (d.struct_bytes != sizeof(mra_gemm_desc)) return "struct_bytes is not sizeof(mra_gemm_desc)";
  if (!d.A || !d.W || !d.C) return "null A, W or C";
  if (d.M <= 0 || d.N <= 0 || d.K <= 0) return "M, N and K must be positive";
  if (d.batch < 0 || d.batch > 65535 || d.a_bs < 0 || d.w_bs < 0 || d.c_bs_bytes < 0 || d.bias_bs < 0) return "negative batch count or batch stride (batch <= 65535)";
  if (d.n_ragged < 0 || d.n_ragged > 1 || d.persist < 0 || d.persist > 1 || d.w_ld < 0 || d.k_rows < 0 || d.w_kwrap < 0 || d.ps_ntiles < 0)
    return "n_ragged and persist are 0 or 1; w_ld, k_rows, w_kwrap and ps_ntiles are not negative";
  if (d.tile_cfg < GT_AUTO || d.tile_cfg >= GEMM_TILES || d.tile_cfg == GT_P8_TAIL) return "tile_cfg outside the forwards' tiles";   // GT_P8_TAIL: no shipped call site
  if (!dbg_view8(d.a_view, &p.a)) return "the A view needs rows per item > 0 and strides that are non-negative multiples of 8";
  if (epi == EPI_KV) p.c = RowView{0, 1, 1};
  else if (!dbg_view(d.c_view, &p.c)) return "the C view needs rows per item > 0 and strides that are non-negative multiples of 4";
  const bool res = epi == EPI_RES_F32 || epi == EPI_RES_LN || epi == EPI_RES_F32_STAT;
  const bool resop = epi == EPI_RES_OP || epi == EPI_RES_OP_STAT, lnf = epi == EPI_LNF_OP || epi == EPI_LNF_GELU_OP;
  if ((resop || lnf || epi == EPI_RES_F32_STAT) && (d.batch > 1 || d.n_ragged)) return "the ViT's epilogues (8, 10 .. 13) take one plain problem: no batch, no n_ragged";
  if (res && (!d.R || !dbg_view(d.r_view, &p.r))) return "the residual needs a pointer and a view with strides that are multiples of 4";
  if (!dbg_aligned(d.A, 16) || !dbg_aligned(d.W, 16) || !dbg_aligned(d.C, 16) || !dbg_aligned(d.bias, 16) || (res && !dbg_aligned(d.R, 16)))
    return "A, W, C, R and bias must be 16-byte aligned";
  if (d.batch > 1 && ((d.a_bs & 7) || (d.w_bs & 7) || (d.c_bs_bytes & 15) || (d.bias_bs & 3)))
    return "batch strides: a_bs and w_bs multiples of 8 elements, c_bs_bytes of 16 bytes, bias_bs of 4 floats";
  if (d.batch > 1 && (epi == EPI_KV || epi == EPI_RES_LN)) return "EPI_KV and EPI_RES_LN take no batch";
  if (p.a.ld < d.K) return "A row stride below K";
  if (d.w_ld && d.w_ld < d.N) return "w_ld below N";
  p.A = d.A; p.W = d.W; p.bias = d.bias; p.C = d.C; p.R = res ? d.R : nullptr;
  p.M = d.M; p.N = d.N; p.K = d.K;
  p.kv_tokens = d.kv_tokens; p.kv_items = d.kv_items; p.kv_heads = d.kv_heads;
  p.batch = d.batch; p.a_bs = d.a_bs; p.w_bs = d.w_bs; p.c_bs_bytes = d.c_bs_bytes; p.bias_bs = d.bias_bs;
  p.n_ragged = d.n_ragged; p.w_ld = d.w_ld; p.k_rows = d.k_rows; p.w_kwrap = d.w_kwrap;
  p.tile_cfg = d.tile_cfg; p.persist = d.persist;
  if (d.k128 < 0 || d.k128 > 1 || d.ps_stats < 0 || d.ps_stats > 1) return "k128 and ps_stats are 0 or 1";
  if (d.ps_stats) {   // P . enc fed by the scores launch's tile statistics: stat_m / stat_l in, no pscale
    if (epi != EPI_OP || d.pscale || !d.w_ld) return "ps_stats goes with EPI_OP over K-major weights (w_ld) and without pscale";
    if (!d.stat_m || !d.stat_l || !dbg_aligned(d.stat_m, 4) || !dbg_aligned(d.stat_l, 4)) return "ps_stats needs stat_m and stat_l (4-byte aligned)";
    if (d.M > 384 || d.ps_ntiles <= 0) return "ps_stats needs M <= 384 (one row tile) and ps_ntiles > 0";
    p.stat_m = d.stat_m; p.stat_l = d.stat_l; p.ps_stats = 1; p.ps_ntiles = d.ps_ntiles;
  }
  if (d.k128 && (d.tile_cfg != GT_64 || d.K % 128)) return "k128 goes with tile_cfg GT_64 and K % 128 == 0";
  p.k128 = d.k128;
  if (epi == EPI_KV) {
    if (d.kv_tokens <= 0 || d.kv_items <= 0 || d.kv_heads <= 0 || d.kv_heads > 1024) return "EPI_KV needs kv_tokens, kv_items and kv_heads > 0";
    if (d.N % (d.kv_heads * 64)) return "EPI_KV: N must be a multiple of kv_heads * 64";
    if ((long long)d.M > (long long)d.kv_items * d.kv_tokens) return "EPI_KV: M exceeds kv_items * kv_tokens";
  }
  if (epi == EPI_RES_LN) {
    if (!d.ln_gain || !d.ln_bias || !d.ln_counter || (!d.ln_y32 && !d.ln_y16)) return "EPI_RES_LN needs gain, bias, counters and an output";
    if ((d.ln_y32 && !dbg_view(d.ln_y32_view, &p.ln_y32v)) || (d.ln_y16 && !dbg_view(d.ln_y16_view, &p.ln_y16v)))
      return "a LayerNorm output view needs rows per item > 0 and strides that are multiples of 4";
    if (!dbg_aligned(d.ln_gain, 16) || !dbg_aligned(d.ln_bias, 16) || !dbg_aligned(d.ln_y32, 16) || !dbg_aligned(d.ln_y16, 16) || !dbg_aligned(d.ln_counter, 4))
      return "the LayerNorm buffers must be 16-byte aligned (counters: 4)";
    if (!(d.ln_eps >= 0.f)) return "ln_eps must not be negative";
    p.ln_gain = d.ln_gain; p.ln_bias = d.ln_bias; p.ln_eps = d.ln_eps; p.ln_y32 = d.ln_y32; p.ln_y16 = d.ln_y16; p.ln_counter = d.ln_counter;
  }
  if (resop) {   // the residual in the operand dtype, addressed like C; in place (aux == C) or apart from it (dbg_gemm_footprint)
    if (!d.aux || !dbg_aligned(d.aux, 16)) return "EPI_RES_OP / EPI_RES_OP_STAT need aux (16-byte aligned)";
    p.aux = d.aux;
  }
  if (epi == EPI_RES_F32_STAT || epi == EPI_RES_OP_STAT) {   // ln_y32: the group statistics, written as float2
    if (!d.ln_y32 || !dbg_aligned(d.ln_y32, 8)) return "the statistics epilogues need ln_y32 (8-byte aligned)";
    if (!d.bias) return "the statistics epilogues need a bias";
    p.ln_y32 = d.ln_y32;
  }
  if (epi == EPI_RES_F32_STAT) {
    if (!d.ln_y16 || !dbg_aligned(d.ln_y16, 16) || !dbg_view8(d.ln_y16_view, &p.ln_y16v))
      return "EPI_RES_F32_STAT needs ln_y16 (16-byte aligned) and a view of it with strides that are multiples of 8";
    p.ln_y16 = d.ln_y16;
  }
  if (lnf) {   // ln_y32: (mean, rstd) per row, read as float2; ln_gain: the column sums of W'
    if (!d.ln_y32 || !dbg_aligned(d.ln_y32, 8)) return "EPI_LNF_* need ln_y32 = (mean, rstd) per row (8-byte aligned)";
    if (!d.ln_gain || !dbg_aligned(d.ln_gain, 16)) return "EPI_LNF_* need ln_gain = the column sums (16-byte aligned)";
    p.ln_y32 = d.ln_y32; p.ln_gain = d.ln_gain;
  }
  if (epi == EPI_SOFTPART) {
    if (!d.stat_m || !d.stat_l || !dbg_aligned(d.stat_m, 4) || !dbg_aligned(d.stat_l, 4)) return "EPI_SOFTPART needs stat_m and stat_l (4-byte aligned)";
    if (!(d.alpha > 0.f) || !(d.alpha < 3.0e38f)) return "EPI_SOFTPART needs a finite alpha > 0";
    p.alpha = d.alpha; p.stat_m = d.stat_m; p.stat_l = d.stat_l;
  }
  if (d.pscale) {
    if (!dbg_aligned(d.pscale, 16)) return "pscale must be 16-byte aligned";
    if (d.M > 384) return "pscale needs M <= 384 (one row tile)";
    p.pscale = d.pscale; p.ps_ntiles = d.ps_ntiles;
  }
  if (d.col_scale || d.col_stats) {
    if (epi != EPI_SOFTPART) return "col_scale belongs to EPI_SOFTPART";
    if (!d.col_scale || !dbg_aligned(d.col_scale, 4)) return "col_scale must be given (4-byte aligned) with col_stats";
    if (d.col_stats < 0 || d.col_stats > 1 || d.cs_bs < 0 || !(d.cs_eps >= 0.f)) return "col_stats is 0 or 1; cs_bs and cs_eps are not negative";
    if (d.batch > 1 && d.cs_bs < d.N) return "cs_bs below N";
    p.col_scale = d.col_scale; p.cs_bs = d.cs_bs; p.col_stats = d.col_stats; p.cs_eps = d.cs_eps;
  }
  return nullptr;
}

const char* dbg_gemm_epi_ok(int epi) {
  switch (epi) {
    case EPI_OP: case EPI_GELU_OP: case EPI_RES_F32: case EPI_F32: case EPI_KV: case EPI_SOFTPART: case EPI_RES_LN: return nullptr;
    case EPI_RES_OP: case EPI_RES_F32_STAT: case EPI_LNF_OP: case EPI_LNF_GELU_OP: case EPI_RES_OP_STAT: return nullptr;   // the ViT encoder's
  }
  return "epilogue must be one of 0 .. 5 and 8 .. 13 (csrc/kernels.h): the training step's EPI_GELU_BOTH / EPI_GELU_BWD have an entry of their own";
}

// weight rows (output columns) of a family's tile: what n_ragged and EPI_SOFTPART round the written columns up to (the kTiles table of gemm.hip)
int dbg_tile_cols(int family) {
  switch (family) {
    case GF_V1_64: case GF_K128_64x128: case GF_K128_64x64: return 64;
    case GF_V1_128: case GF_WS_128x384: case GF_P8_TAIL: return 128;
    case GF_V1_256: case GF_WS_256: case GF_P8_256: case GF_P8_MIXED: return 256;
    case GF_WS_176x384: return 176;
    case GF_RING_144x128: return 144;
    case GF_RING_192x128: return 192;
    case GF_RING_96x64: return 96;
  }
  return 0;
}

// the read and write footprint of problem d under the plan's tile against the sizes the caller gave
const char* dbg_gemm_footprint(const mra_gemm_desc& d, const GemmProb& p, const GemmPlan& pl, int g, int epi) {
  const long long nb = d.batch > 1 ? d.batch : 1;
  const long long ntiles = pl.args.p[g].ntiles;
  const long long cols = (d.n_ragged || epi == EPI_SOFTPART) ? ntiles * dbg_tile_cols(pl.family) : d.N;   // columns of C a tile row writes
  const size_t csz = (epi == EPI_RES_F32 || epi == EPI_F32 || epi == EPI_RES_LN || epi == EPI_RES_F32_STAT) ? 4 : 2;
  if ((d.n_ragged || epi == EPI_SOFTPART) && (cols < d.N || ntiles != (d.N + dbg_tile_cols(pl.family) - 1) / dbg_tile_cols(pl.family))) return "unknown tile";
  if (!dbg_fits(dbg_extent(p.a, d.M, d.K) + (u128)(nb - 1) * (u128)d.a_bs, 2, 0, d.a_bytes)) return "A: the view, K and the batch stride leave a_bytes";
  u128 w = d.w_ld ? (u128)(d.k_rows - 1) * (u128)d.w_ld + (u128)d.N : (u128)d.N * (u128)(d.w_kwrap ? d.K / 2 : d.K);
  if (!dbg_fits(w + (u128)(nb - 1) * (u128)d.w_bs, 2, 0, d.w_bytes)) return "W: N, K (w_ld, k_rows, w_kwrap) and the batch stride leave w_bytes";
  if (d.bias && !dbg_fits((u128)d.N + (u128)(nb - 1) * (u128)d.bias_bs, 4, 0, d.bias_bytes)) return "bias: N and the batch stride leave bias_bytes";
  if (epi == EPI_KV) {
    const u128 n = (u128)(d.N / (d.kv_heads * 64)) * (u128)d.kv_items * (u128)d.kv_heads * (u128)d.kv_tokens * 64;
    if (!dbg_fits(n, 2, 0, d.c_bytes)) return "C: the head-major scatter leaves c_bytes";
  } else {
    if (p.c.ld < cols) return "C row stride below the columns written (ceil(N / tile) * tile with n_ragged and EPI_SOFTPART)";
    if (!dbg_fits(dbg_extent(p.c, d.M, cols), csz, (u128)(nb - 1) * (u128)d.c_bs_bytes, d.c_bytes)) return "C: the view, the columns written and the batch stride leave c_bytes";
  }
  if (p.R) {
    if (p.r.ld < d.N) return "R row stride below N";
    if (!dbg_fits(dbg_extent(p.r, d.M, d.N), 4, 0, d.r_bytes)) return "R: the view leaves r_bytes";
  }
  if (p.aux) {   // addressed with C's view: the same footprint; the stream updated in place is the one overlap a tile's read-then-write order allows
    if (!dbg_fits(dbg_extent(p.c, d.M, cols), 2, 0, d.aux_bytes)) return "aux: the C view and the columns written leave aux_bytes";
    const uintptr_t c0 = (uintptr_t)d.C, a0 = (uintptr_t)d.aux;
    const u128 span = dbg_extent(p.c, d.M, cols) * 2;
    if (a0 != c0 && (u128)a0 < (u128)c0 + span && (u128)c0 < (u128)a0 + span) return "aux overlaps C without being C";
  }
  if (epi == EPI_RES_F32_STAT || epi == EPI_RES_OP_STAT) {
    const int gw = epi == EPI_RES_F32_STAT ? 128 : 64;
    if (d.N % gw) return "the statistics epilogues need N to be a multiple of the group width (128 in fp32, 64 in the operand dtype)";
    if (!dbg_fits((u128)d.M * (u128)(d.N / gw) * 2, 4, 0, d.ln_y32_bytes)) return "ln_y32: M x (N / group width) x 2 floats leave ln_y32_bytes";
  }
  if (epi == EPI_RES_F32_STAT && (p.ln_y16v.ld < d.N || !dbg_fits(dbg_extent(p.ln_y16v, d.M, d.N), 2, 0, d.ln_y16_bytes)))
    return "ln_y16: row stride below N, or the view leaves ln_y16_bytes";
  if (epi == EPI_LNF_OP || epi == EPI_LNF_GELU_OP) {
    if (!dbg_fits((u128)d.M * 2, 4, 0, d.ln_y32_bytes)) return "ln_y32: M x 2 floats of (mean, rstd) leave ln_y32_bytes";
    if (!dbg_fits((u128)d.N, 4, 0, d.ln_gain_bytes)) return "ln_gain: N floats of column sums leave ln_gain_bytes";
  }
  if (epi == EPI_SOFTPART) {
    const u128 n = (u128)nb * (u128)d.M * (u128)ntiles;
    if (!dbg_fits(n, 4, 0, d.stat_m_bytes) || !dbg_fits(n, 4, 0, d.stat_l_bytes)) return "stat_m / stat_l: batch * M * ntiles floats leave their sizes";
  }
  if (p.ps_stats) {
    const u128 n = (u128)nb * (u128)d.M * (u128)d.ps_ntiles;
    if (!dbg_fits(n, 4, 0, d.stat_m_bytes) || !dbg_fits(n, 4, 0, d.stat_l_bytes)) return "ps_stats: batch * M * ps_ntiles floats of stat_m / stat_l leave their sizes";
  }
  if (p.pscale && !dbg_fits((u128)nb * (u128)d.ps_ntiles * 512, 4, 0, d.pscale_bytes)) return "pscale: batch * ps_ntiles * 512 floats leave pscale_bytes";
  if (p.col_scale && !dbg_fits((u128)d.N + (u128)(nb - 1) * (u128)d.cs_bs, 4, 0, d.col_scale_bytes)) return "col_scale: N floats and the batch stride leave col_scale_bytes";
  if (epi == EPI_RES_LN) {
    if (!dbg_fits((u128)d.N, 4, 0, d.ln_gain_bytes) || !dbg_fits((u128)d.N, 4, 0, d.ln_bias_bytes)) return "ln_gain / ln_bias: N floats leave their sizes";
    if (p.ln_y32 && (p.ln_y32v.ld < d.N || !dbg_fits(dbg_extent(p.ln_y32v, d.M, d.N), 4, 0, d.ln_y32_bytes))) return "ln_y32: row stride below N, or the view leaves ln_y32_bytes";
    if (p.ln_y16 && (p.ln_y16v.ld < d.N || !dbg_fits(dbg_extent(p.ln_y16v, d.M, d.N), 2, 0, d.ln_y16_bytes))) return "ln_y16: row stride below N, or the view leaves ln_y16_bytes";
    if (!dbg_fits((u128)((d.M + 63) / 64), 4, 0, d.ln_counter_bytes)) return "ln_counter: ceil(M / 64) counters leave ln_counter_bytes";
  }
  return nullptr;
}

// descriptors -> problems + plan; every refusal of mra_debug_gemm (none needs a device: mra_debug_gemm_plan makes the same).  0 or MRA_EINVAL (message set).
int dbg_gemm_prepare(const mra_gemm_desc* probs, int32_t nprob, int32_t epi, int32_t dtype, int cus, GemmProb* ps, GemmPlan* pl, int* op) {
  if (nprob < 1 || nprob > GEMM_MAX_GROUPS) return fail(MRA_EINVAL, "1 .. 4 problems");
  if (!dbg_op(dtype, op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (const char* e = dbg_gemm_epi_ok(epi)) return fail(MRA_EINVAL, e);
  if (nprob > 1 && (epi == EPI_RES_OP || epi >= EPI_RES_F32_STAT)) return fail(MRA_EINVAL, "the ViT's epilogues (8, 10 .. 13) take one problem");
  if (!probs) return fail(MRA_EINVAL, "null descriptor array");
  for (int i = 0; i < nprob; ++i)
    if (const char* e = dbg_gemm_prob(probs[i], epi, &ps[i])) return fail(MRA_EINVAL, "problem " + std::to_string(i) + ": " + e);
  pl->cus = cus;
  const int rc = gemm_plan(ps, nprob, epi, *op, pl);
  if (rc) return fail(MRA_EINVAL, rc == -2 ? "the tile has no such epilogue" : "gemm_plan refuses the launch (K % 64, K % 128 on the 128-deep and eight-phase tiles, N % tile, N % 256 == 128 and N >= 384 on the mixed tile, what the tile or the epilogue allows)");
  for (int i = 0; i < nprob; ++i)
    if (const char* e = dbg_gemm_footprint(probs[i], ps[i], *pl, i, epi)) return fail(MRA_EINVAL, "problem " + std::to_string(i) + ": " + e);
  if (epi == EPI_RES_LN)
    for (int i = 0; i < nprob; ++i)
      for (int j = i + 1; j < nprob; ++j) {
        const uintptr_t a0 = (uintptr_t)ps[i].ln_counter, a1 = a0 + 4 * (uintptr_t)((ps[i].M + 63) / 64);
        const uintptr_t b0 = (uintptr_t)ps[j].ln_counter, b1 = b0 + 4 * (uintptr_t)((ps[j].M + 63) / 64);
        if (a0 < b1 && b0 < a1) return fail(MRA_EINVAL, "the counter ranges of two EPI_RES_LN problems overlap");
      }
  return MRA_OK;
}
}  // namespace

int mra_debug_gemm(const mra_gemm_desc* probs, int32_t nprob, int32_t epilogue, int32_t dtype, void* stream) {
  GemmProb ps[GEMM_MAX_GROUPS];
  static thread_local GemmPlan pl;   // (a plan carries the kernel argument: ~2 KB)
  int op;
  if (const int rc = dbg_gemm_prepare(probs, nprob, epilogue, dtype, 0, ps, &pl, &op)) return rc;
  return chk(launch_gemm(ps, nprob, epilogue, op, as_stream(stream)), "debug gemm");
}

int mra_debug_kvgrad_gemm(mra_qformer* h, const void* dkv, size_t dkv_bytes, int32_t enc_items, int32_t kv, float* d_enc, size_t d_enc_bytes,
                          void* stream) {
  if (enc_items < 0 || kv < 0) return fail(MRA_EINVAL, "negative size");
  if (enc_items > 0 && kv > 0 && (!dkv || !d_enc)) return fail(MRA_EINVAL, "null dkv or d_enc");
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (enc_items == 0 || kv == 0) return MRA_OK;
  if (h->ncross <= 0) return fail(MRA_ESTATE, "the handle has no cross-attention layer");
  if ((long long)enc_items * kv > 0x7fffffffLL - 64) return fail(MRA_EINVAL, "enc_items * kv exceeds int32");
  if (!dbg_aligned(dkv, 16) || !dbg_aligned(d_enc, 4)) return fail(MRA_EINVAL, "dkv must be 16-byte aligned (d_enc: 4)");
  // footprints: the whole head-major cache [ncross * 2][enc_items][heads][kv][64] is read, [enc_items * kv][E] floats are written
  const size_t rows = (size_t)enc_items * kv;
  const size_t need_dkv = (size_t)h->ncross * 2 * rows * h->cfg.hidden * 2, need_out = rows * h->cfg.enc_width * 4;
  if (dkv_bytes < need_dkv) return fail(MRA_EINVAL, "dkv_bytes below the cache's footprint of " + std::to_string(need_dkv) + " bytes");
  if (d_enc_bytes < need_out) return fail(MRA_EINVAL, "d_enc_bytes below the output's footprint of " + std::to_string(need_out) + " bytes");
  return chk(launch_kvgrad_gemm(dkv, h->wkv, d_enc, enc_items, kv, h->cfg.heads, h->ncross * 2, h->cfg.enc_width, h->op(), as_stream(stream)),
             "kvgrad gemm");
}

int mra_debug_gemm_plan(const mra_gemm_desc* probs, int32_t nprob, int32_t epilogue, int32_t dtype, int32_t cus, int32_t* out) {
  GemmProb ps[GEMM_MAX_GROUPS];
  static thread_local GemmPlan pl;
  int op;
  if (!out) return fail(MRA_EINVAL, "null out");
  if (cus < 0) return fail(MRA_EINVAL, "negative cus");
  if (const int rc = dbg_gemm_prepare(probs, nprob, epilogue, dtype, cus, ps, &pl, &op)) return rc;
  const int32_t r[7] = {pl.tile, pl.family, pl.threads, pl.lds, pl.grid, pl.persistent, pl.args.total_tiles};
  for (int i = 0; i < 7; ++i) out[i] = r[i];
  return MRA_OK;
}

// The fused query launch of the folded cross-attention (fold.hip: fold_query_kernel; "cross_fuse" bit 1) on its own, through the launch function
// the forward calls.  Every null, misaligned or short buffer is refused before anything is launched; nothing is allocated.
int mra_debug_fold_query(const void* x, const int64_t* x_view, size_t x_bytes, const void* w_q, size_t w_q_bytes, const float* b_q, size_t b_q_bytes,
                         const void* w_k, size_t w_k_bytes, void* q_prime, size_t q_prime_bytes, int32_t rows, int32_t H, int32_t E, int32_t Q,
                         int32_t heads, int32_t dtype, void* stream) {
  int op;
  if (rows < 0) return fail(MRA_EINVAL, "negative rows");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (H < 64 || H % 64 || E < 64 || E % 64 || Q <= 0 || heads <= 0 || heads > 1024 || rows % Q)
    return fail(MRA_EINVAL, "need H and E positive multiples of 64, Q > 0, 0 < heads <= 1024, rows % Q == 0");
  RowView xv;
  if (!dbg_view8(x_view, &xv) || xv.ld < H) return fail(MRA_EINVAL, "bad row view of x: strides multiples of 8, row stride >= H");
  if (rows == 0) return MRA_OK;
  if (!x || !w_q || !w_k || !q_prime) return fail(MRA_EINVAL, "null argument");
  if (!dbg_aligned(x, 16) || !dbg_aligned(w_q, 16) || !dbg_aligned(w_k, 16) || !dbg_aligned(q_prime, 16) || !dbg_aligned(b_q, 16))
    return fail(MRA_EINVAL, "misaligned buffer");
  if (!dbg_fits(dbg_extent(xv, rows, H), 2, 0, x_bytes)) return fail(MRA_EINVAL, "x: the view and H leave x_bytes");
  if (!dbg_fits((u128)heads * 64 * (u128)H, 2, 0, w_q_bytes)) return fail(MRA_EINVAL, "w_q: heads * 64 rows of H leave w_q_bytes");
  if (b_q && !dbg_fits((u128)heads * 64, 4, 0, b_q_bytes)) return fail(MRA_EINVAL, "b_q: heads * 64 floats leave b_q_bytes");
  if (!dbg_fits((u128)heads * (u128)E * 64, 2, 0, w_k_bytes)) return fail(MRA_EINVAL, "w_k: heads blocks of [E][64] leave w_k_bytes");
  if (!dbg_fits((u128)rows * (u128)heads * (u128)E, 2, 0, q_prime_bytes)) return fail(MRA_EINVAL, "q_prime: rows * heads * E elements leave q_prime_bytes");
  return chk(launch_fold_query(x, xv, w_q, b_q, w_k, q_prime, rows, H, E, Q, heads, op, as_stream(stream)), "fold_query");
}

int64_t mra_debug_fold_query_launches(void) { return fold_query_launch_count(); }
int64_t mra_debug_fold_rowfactor_launches(void) { return fold_rowfactor_launch_count(); }

// Steps 1 + 2 of a layer in ONE launch (attention.hip: qkv_attn_kernel; "self_fuse") on its own, through the launch function the forward calls;
// hidden = heads * 64.  Shapes outside the plan (S > 64) are refused, nothing is launched.
int mra_debug_qkv_attention(const void* rows, const void* wqkv, const float* bqkv, const int64_t* mask, int32_t dtype, int32_t items, int32_t S,
                            int32_t heads, void* ctx, void* stream) {
  int op;
  if (items < 0 || S < 1 || heads < 1 || heads > 16) return fail(MRA_EINVAL, "sizes: items >= 0, S >= 1, heads in 1..16");
  if (!dbg_op(dtype, &op)) return fail(MRA_EINVAL, "dtype must be f16 or bf16");
  if (!qkv_attn_supported(S, heads * 64, heads)) return fail(MRA_EINVAL, "the fused launch takes S <= 64 (longer prompts run the two launches)");
  if (items == 0) return MRA_OK;
  if (!rows || !wqkv || !ctx) return fail(MRA_EINVAL, "null argument");
  if (!dbg_aligned(rows, 16) || !dbg_aligned(wqkv, 16) || !dbg_aligned(ctx, 16) || !dbg_aligned(bqkv, 16))
    return fail(MRA_EINVAL, "rows, wqkv, bqkv and ctx must be 16-byte aligned");
  return chk(launch_qkv_attention(rows, wqkv, bqkv, (const long long*)mask, ctx, items, S, heads * 64, heads, op, as_stream(stream)), "qkv + self attention");
}
int64_t mra_debug_qkv_attention_launches(void) { return qkv_attn_launch_count(); }
int64_t mra_debug_attention_launches(int32_t masked) { return attn_launch_count(masked); }
// 1: a forward with `lanes` lanes of `items` items at S rows each takes the fused launch under the option values given; 0: it keeps the two launches
int32_t mra_debug_self_fuse_plan(int32_t option, int32_t chain_ring, int32_t lanes, int32_t items, int32_t S, int32_t hidden, int32_t heads,
                                 int32_t dtype, int32_t want_full) {
  int op;
  if (!dbg_op(dtype, &op) || items < 0 || S < 0) return 0;
  return self_fuse_plan(option, lanes, (long long)items * S, S, hidden, heads, op, chain_ring, want_full != 0) ? 1 : 0;
}

}  // extern "C"
