// Private to the library: the handle behind include/mra.h, its parameter registry and small host helpers
// shared by the inference path (mra_abi.hip), the training path (mra_train.hip) and the attached LM's entries (mra_lm.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/mra.h"
#include "kernels.h"
#include "mra_common.h"

namespace mra_host {

using namespace mra;

extern thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess) return fail(MRA_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }
inline size_t up256(size_t n) { return (n + 255) / 256 * 256; }
inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
inline bool aligned4(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

struct Param {
  void* ptr = nullptr;   // destination inside the arena
  int dtype = MRA_F32;   // stored dtype
  long long numel = 0;   // elements expected from the source tensor
  bool loaded = false;
  size_t goff = 0;       // byte offset of this parameter's f32 gradient in the flat gradient buffer
  int rows = 0, cols = 0;  // matrix shape ([out, in]) for weights, 0 otherwise
  float* copy32 = nullptr;  // f32 copy kept beside the operand-dtype one (the score-chain weights of the split-precision cross-attention)
  int store = 0;            // encoders: 0 = convert to `dtype` at ptr, otherwise the handle's own store kind (a repacking kernel)
  bool required = true;     // encoders: counts as missing until loaded
};
using Registry = std::map<std::string, Param>;

struct LayerW {
  void *wqkv, *wo, *wcq, *wco, *wiq, *woq, *wit, *wot;
  float *bqkv, *bo, *bcq, *bco, *biq, *boq, *bit, *bot;
  float *ln1g, *ln1b, *lncg, *lncb, *lnqg, *lnqb, *lntg, *lntb;
  float* wcq32;     // f32 copy of the cross-attention query weight (split-precision cross-attention), cross layers only
  int cross_index;  // -1 when the layer has no cross-attention
  // transposed copies for the data-gradient GEMMs (training only; nullptr until mra_qformer_enable_training)
  void *wqkvT, *woT, *wcqT, *wcoT, *wiqT, *woqT, *witT, *wotT;
};

struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(char* b) : base(b) {}
  template <typename T>
  T* take(size_t count, size_t elem = sizeof(T)) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += align_up(count * elem);
    return p;
  }
};

inline RowView plain(int rows, int ld) { return RowView{0, rows > 0 ? rows : 1, ld}; }
inline RowView items_view(long long item_stride, int rpi, int ld) { return RowView{item_stride, rpi, ld}; }
inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline int chk(int rc, const char* what) {
  if (rc == 0) return 0;
  return fail(rc == -1 ? MRA_EINVAL : MRA_EHIP, std::string(what) + " failed (rc " + std::to_string(rc) + ")");
}

// ---- the encoder handles (mra_vit, mra_beats): parameters are registered by name while the arena is laid out (as mra_qformer's), and
// `load` is look-up + size check + one switch over the few store kinds ----
// A per-layer name ("<layer_prefix><i>.<rest>") with a bad index is told from a bad name; the index is read as atoi reads it.
inline Param* find_param(Registry& reg, const std::string& key, const std::string& layer_prefix, int nlayers) {
  auto it = reg.find(key);
  if (it == reg.end() && key.rfind(layer_prefix, 0) == 0) {
    const size_t p0 = layer_prefix.size(), dot = key.find('.', p0);
    if (dot != std::string::npos) {
      const int li = atoi(key.substr(p0, dot - p0).c_str());
      if (li < 0 || li >= nlayers) { fail(MRA_ENAME, "layer index out of range: " + key); return nullptr; }
      it = reg.find(layer_prefix + std::to_string(li) + key.substr(dot));
    }
  }
  if (it == reg.end()) { fail(MRA_ENAME, "unknown parameter name: " + key); return nullptr; }
  return &it->second;
}
inline int check_numel(const std::string& key, const Param& pr, const int64_t* shape, int ndim) {
  long long numel = 1;
  for (int i = 0; i < ndim; ++i) numel *= shape[i];
  return numel == pr.numel ? 0 : fail(MRA_EINVAL, "parameter " + key + ": expected " + std::to_string(pr.numel) + " elements, got " + std::to_string(numel));
}
inline int count_missing(const Registry& reg) {
  int n = 0;
  for (auto& kv : reg) n += kv.second.required && !kv.second.loaded;
  return n;
}
// device -> size pass -> hipMalloc -> layout pass -> memset (padding and optional parameters stay zero); `layout(h, base)` lays h's arena out
// at base (nullptr: only measures) and returns its size.  On failure nothing is left allocated; the caller deletes h.
template <typename H, typename Layout>
int create_arena(H* h, Layout layout, const char* what) {
  HIP_TRY(hipGetDevice(&h->device));
  h->arena_bytes = layout(h, nullptr);
  hipError_t e = hipMalloc((void**)&h->arena, h->arena_bytes);
  if (e != hipSuccess) { h->arena = nullptr; return fail(MRA_ENOMEM, std::string("hipMalloc of the ") + what + " parameter arena: " + hipGetErrorString(e)); }
  layout(h, h->arena);
  e = hipMemsetAsync(h->arena, 0, h->arena_bytes, 0);
  if (e != hipSuccess) { (void)hipFree(h->arena); h->arena = nullptr; return fail(MRA_EHIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e)); }
  return MRA_OK;
}

// f(T{}) with T the I-th of Ts (the last one for any larger I): a run-time dtype code as a compile-time element type, e.g.
//   with_op(op, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(kernel<T>, ...); });
template <typename T0, typename... Ts, typename F>
auto with_type(int i, F&& f) {
  if constexpr (sizeof...(Ts) == 0) return f(T0{});
  else return i == 0 ? f(T0{}) : with_type<Ts...>(i - 1, f);
}
template <typename F> auto with_op(int op, F&& f) { return with_type<f16, bf16>(op, f); }                 // OP_F16 / OP_BF16
template <typename F> auto with_src(int dtype, F&& f) { return with_type<float, f16, bf16>(dtype, f); }   // MRA_F32 / MRA_F16 / MRA_BF16
template <typename F> auto with_f32_f16(int dtype, F&& f) { return with_type<float, f16>(dtype, f); }     // inputs that are f32 or f16 only

}  // namespace mra_host

struct mra_qformer {
  mra_cfg cfg;
  int device = 0;
  int ncross = 0;
  char* arena = nullptr;
  size_t arena_bytes = 0;
  std::map<std::string, mra_host::Param> params;
  std::vector<mra_host::LayerW> layers;
  // embeddings / extras
  float *word = nullptr, *pos = nullptr, *embg = nullptr, *embb = nullptr, *query = nullptr;
  float *encg = nullptr, *encb = nullptr;
  void* wkv = nullptr;  // [ncross*2*H, E]
  float* bkv = nullptr;
  void* wllm = nullptr;
  float* bllm = nullptr;
  // folded cross-attention (mra_qformer_set_cross_mode): per cross layer the key weight regrouped as [heads][E][64]
  // ... and, behind those, the weights of the raw-feature form (mra_qformer_forward_raw): per cross layer the key weight with the modality
  // LayerNorm folded in, W_k diag(g) centred over E, in the same [heads][E][64] layout; the value weight likewise as [H][E]; and the
  // value bias b_v + W_v b (mra_host::fold_raw_*).  Rebuilt with the regrouped key weights whenever a parameter is loaded (fold_stale).
  char* arena_f = nullptr;
  bool fold_stale = true;
  bool raw_features = true;                       // mra_qformer_set_option "raw_features": 0 = mra_qformer_raw_features_ok answers no (A/B)
  bool inreg_rescale = true;                      // the P . enc GEMM applies the softmax row factors to its P~ fragments (false: a rescale pass over P; cross mode 5)
  int fold_tile = mra::GT_128;                    // GemmTile of the two batched GEMMs where the 176 x 384 tiles do not apply (GT_128 or GT_WS_128x384)
  bool fold_stream = false;                       // folded path on the streaming kernels of fold_stream.hip (mra_qformer_set_cross_mode 4)
  int cross_mode = 0;                             // 0 automatic, 1 K/V cache, 2 folded
  // split-precision cross-attention (mra_qformer_set_cross_precision): hidden state, W_cq, Q, W_k and Q' of the score chain as operand-dtype
  // hi + lo pairs (folded form forced); wk32 = f32 copies of the key weights [ncross][H][E], arena_p = per cross layer W_cq as
  // [H][3H] (hi | hi | lo) and W_k as [heads][E][192] (hi | hi | lo), allocated when the mode is first enabled
  // layer-chain GEMMs on the ring kernel's exact-fit tiles (mra_qformer_set_option "chain_ring"): bit 0 QKV (144 x 128), bit 1 FFN-up (192 x 128),
  // bit 2 the N = hidden projections with a residual (96 x 64), bit 3 (with bit 2) their LayerNorm inside the same launch (EPI_RES_LN: measured
  // SLOWER in the step -- 6.95 vs 6.73-6.93 ms, reference item shape 2.86-2.92 vs 2.65-2.83 -- opt-in); chosen per launch only where the tile
  // divides N and the launch has >= ~1 k rows
  int chain_ring = 7;    // measured in the step (r03d, same box): mask 0 / 1 / 3 / 7 = 6.65 / 6.64 / 6.59 / 6.56 ms; reference item shape 2.55 / 2.62 / - / 2.52 ms
  int train_ring = 4;   // the same mask for the training forward / backward GEMMs (mra_qformer_set_option "train_ring"): bit 0 QKV, bit 2 every N = hidden
                        // GEMM whose epilogue the ring kernel has (projections with a residual, the data gradients).  Measured at B = 1 x T = 20 (r03x,
                        // one session): 14.6-15.2 ms per step with 0, 14.0-14.3 with 4, 14.2 with 5
  // folded cross-attention, default plan only (mra_qformer_set_option "cross_fuse"): bit 1 = cross query projection and Q' in one launch
  // (fold.hip: fold_query_kernel, bit-identical to the two GEMM launches); bit 4 = the per-head context GEMM on the 64 x 64 tile with 128-deep
  // K steps (192 workgroups that pull 360 KB each instead of 96 that pull 540 KB; bit-identical too); bit 2 = the row factors computed inside
  // the P . enc launch from the scores launch's tile statistics (GemmProb::ps_stats: no fold_rowfactor launch, no factor array; bit-identical,
  // but that launch grows by 61 us to save 11: measured slower, opt-in only); 0 = the launches as they were
  int cross_fuse = 1;   // measured in the step, one process, masks in turn: 0 / 1 / 2 / 3 / 4 / 7 = 6.463 / 6.380 / 6.760 / 6.675 / 6.460 / 6.668 ms
  // steps 1 + 2 of a layer (QKV projection, masked self-attention) in ONE launch (mra_qformer_set_option "self_fuse"; attention.hip:
  // qkv_attn_kernel, bit-identical to the two launches, qkv16 neither written nor read): single-lane forwards with S <= 64, 64-wide heads and
  // the QKV GEMM on its ring tile (>= 1024 rows); the pair forward, longer prompts, smaller forwards and the training forward keep the two launches
  int self_fuse = 1;    // measured in the step, parent / this build alternating: 6.4095 -> 6.303 ms and, a second session, 6.520 -> 6.440 ms; reference item shape 2.616 -> 2.452 ms
  // mra_qformer_forward_multi: the cross core that lets several prompts read one K/V stream (mra_qformer_set_option "multi_core"):
  // 0 attn_kernel with AttnArgs::kv_share, 1 the shared-stream core (attn_shared_kernel).  The rule for the default: whichever the line of
  // tools/bench_multi_query.py shows faster at P >= 4 on both of its shapes.  Measured (profiles/multi_query_line.json, one session): 1 at
  // every P >= 4 -- 40 x Kv 257: 4.73 / 8.65 / 16.40 ms against 4.77 / 8.67 / 16.57 at P = 4 / 8 / 16; 32 x Kv 8224: 11.45 / 15.74 against
  // 11.63 / 16.11 at P = 4 / 8 (0.2 - 2.3 %); at P = 2, where half of every workgroup idles, 0 is ahead (Kv 8224: 9.33 against 9.89 ms)
  int multi_core = 1;
  int cross_precise = 0;
  float* wk32 = nullptr;
  char* arena_p = nullptr;
  bool precise_stale = true;
  // automatic precision (mra_qformer_set_cross_precision 2): the first forward after a weight upload runs the op-precision folded chain with
  // the probe variant of the row-factor kernel, which bins every row's softmax maximum p_max = 1 / L into auto_hist [ncross][256]; the largest
  // per-layer median p_max >= auto_tau_milli / 1000 resolves to split (cross_precise = 1), otherwise to op (cross_precise = 0)
  bool cross_auto = false;
  bool auto_stale = true;                         // a probe is pending (set wherever precise_stale is)
  int auto_resolved = -1;                         // 0 op, 1 split, -1 never probed
  int auto_probes = 0;                            // probes run since create
  int auto_tau_milli = 500;                       // mra_qformer_set_option "auto_split_pmax_milli"
  int* auto_hist = nullptr;                       // device histograms [ncross][256]
  int* auto_hist_host = nullptr;                  // pinned host copy
  std::vector<float> auto_median;                 // per cross layer median p_max of the last probe (-1: none yet)
  hipEvent_t kv_done = nullptr;                   // optional scheduling hook (mra_qformer_set_kv_done_event)
  hipEvent_t kv_ev0 = nullptr, kv_ev1 = nullptr;  // optional instrumentation (mra_qformer_set_kv_events)
  // training
  char* arena_t = nullptr;      // transposed weight copies
  bool transposes_stale = true;
  mra::TrJob* tr_jobs = nullptr;   // device table of the batched transpose (built on first use)
  int n_tr_jobs = 0, n_tr_tiles = 0;
  hipStream_t wg_stream = nullptr;                // side stream of the weight-gradient GEMMs (mra_qformer_backward)
  hipEvent_t wg_ev[32] = {};                      // ring of fork / done events between the caller's stream and wg_stream
  // fused optimizer pass (mra_qformer_adam_step): matrices with a transposed training copy as 64 x 64 tile jobs, every other bert.* parameter
  // (and the query tokens) as linear segments, the f32 copies of the score-chain weights as a third table; built by mra_qformer_enable_training
  mra::AdamMatJob* adam_jobs = nullptr;
  int n_adam_jobs = 0, n_adam_tiles = 0;
  mra::FlatSeg* adam_segs = nullptr;
  int n_adam_segs = 0;
  mra::FlatSeg* c32_segs = nullptr;
  int n_c32_segs = 0;
  size_t grad_bytes = 0;
  mra::FlatSeg* flat_segs = nullptr;  // device table behind mra_qformer_load_flat (bert.* parameters)
  int n_flat_segs = 0;
  int op() const { return cfg.op_dtype == MRA_BF16 ? mra::OP_BF16 : mra::OP_F16; }
};

namespace mra_host {
// padded score-row length: whole 128- and 176-row tiles of the scores GEMM, and a multiple of 128 (K of P . enc)
inline int fold_kvp(int kv) { return (std::max((kv + 127) / 128 * 128, (kv + 175) / 176 * 176) + 127) / 128 * 128; }
// raw-feature form: where cross layer ci's folded weights live in arena_f (W_k' | W_v' | value bias), and the arena's size
inline size_t fold_raw_layer_bytes(const mra_qformer* h) { return align_up((size_t)2 * h->cfg.hidden * h->cfg.enc_width * 2 + (size_t)h->cfg.hidden * 4); }
inline size_t fold_raw_off(const mra_qformer* h) { return align_up((size_t)h->ncross * h->cfg.hidden * h->cfg.enc_width * 2); }
inline char* fold_raw_wk(const mra_qformer* h, int ci) { return h->arena_f + fold_raw_off(h) + (size_t)ci * fold_raw_layer_bytes(h); }
inline char* fold_raw_wv(const mra_qformer* h, int ci) { return fold_raw_wk(h, ci) + (size_t)h->cfg.hidden * h->cfg.enc_width * 2; }
inline float* fold_raw_bv(const mra_qformer* h, int ci) { return (float*)(fold_raw_wv(h, ci) + (size_t)h->cfg.hidden * h->cfg.enc_width * 2); }
inline size_t fold_arena_bytes(const mra_qformer* h) { return fold_raw_off(h) + (size_t)h->ncross * fold_raw_layer_bytes(h); }
// split-precision cross-attention: bytes of one cross layer's prepared weights, W_cq [H][3H] then W_k [heads][E][192] (operand dtype)
inline size_t precise_wk_off(const mra_qformer* h) { return align_up((size_t)h->cfg.hidden * 3 * h->cfg.hidden * 2); }
inline size_t precise_layer_bytes(const mra_qformer* h) {
  return precise_wk_off(h) + align_up((size_t)h->cfg.heads * h->cfg.enc_width * 192 * 2);
}
// attention over the packed Q | K | V rows [items][S][3H] of a layer's self-attention; the context leaves as [items][S][H]
inline AttnArgs self_attn_args(const mra_cfg& c, const void* qkv16, void* ctx16, const long long* mask, int items, int S, float* lse = nullptr) {
  const int H = c.hidden;
  AttnArgs a{};
  a.Q = qkv16; a.K = (const char*)qkv16 + (size_t)H * 2; a.V = (const char*)qkv16 + (size_t)2 * H * 2; a.O = ctx16;
  a.q_item_stride = a.k_item_stride = a.v_item_stride = (long long)S * 3 * H; a.q_ld = a.k_ld = a.v_ld = 3 * H;
  a.k_head_stride = a.v_head_stride = 64; a.o_item_stride = (long long)S * H; a.o_ld = H;
  a.mask = mask; a.mask_ld = S;
  a.items = items; a.heads = c.heads; a.q_rows = S; a.kv_len = S; a.scale = 0.125f; a.nsplit = 1; a.lse = lse;
  return a;
}
// its backward: Q, K, V in place in the same packed rows, dQ | dK | dV into rows of the same layout, the context and its gradient [items][S][H]
inline AttnBwdArgs self_attn_bwd_args(const mra_cfg& c, const void* qkv16, const void* ctx16, const void* dctx16, const long long* mask,
                                      const float* lse, int items, int S, void* dqkv16) {
  const int H = c.hidden;
  AttnBwdArgs g{};
  g.Q = qkv16; g.K = (const char*)qkv16 + (size_t)H * 2; g.V = (const char*)qkv16 + (size_t)2 * H * 2; g.O = ctx16; g.dO = dctx16;
  g.dQ = dqkv16; g.dK = (char*)dqkv16 + (size_t)H * 2; g.dV = (char*)dqkv16 + (size_t)2 * H * 2;
  g.q_item_stride = g.k_item_stride = g.v_item_stride = g.dq_item_stride = g.dk_item_stride = g.dv_item_stride = (long long)S * 3 * H;
  g.q_ld = g.k_ld = g.v_ld = g.dq_ld = g.dk_ld = g.dv_ld = 3 * H;
  g.k_head_stride = g.v_head_stride = g.dk_head_stride = g.dv_head_stride = 64;
  g.o_item_stride = (long long)S * H; g.o_ld = H;
  g.mask = mask; g.mask_ld = S; g.lse = lse;
  g.items = items; g.heads = c.heads; g.q_rows = S; g.kv_len = S; g.scale = 0.125f;
  return g;
}
// cross-attention core of cross layer ci over the head-major K/V cache [ncross][k | v][items][heads][kv][64]: Q and the context [items][32][H]
inline AttnArgs kv_cross_attn_args(const mra_cfg& c, const void* q16, const char* kv16, int ci, void* ctx16, int items, int kv, int nsplit,
                                   float* part, float* lse = nullptr) {
  const int H = c.hidden, Q = c.n_query;
  const size_t per_sel = (size_t)items * c.heads * kv * 64 * 2;
  AttnArgs a{};
  a.Q = q16; a.K = kv16 + (size_t)(ci * 2 + 0) * per_sel; a.V = kv16 + (size_t)(ci * 2 + 1) * per_sel; a.O = ctx16;
  a.q_item_stride = a.o_item_stride = (long long)Q * H; a.q_ld = a.o_ld = H;
  a.k_item_stride = a.v_item_stride = (long long)c.heads * kv * 64; a.k_head_stride = a.v_head_stride = (long long)kv * 64; a.k_ld = a.v_ld = 64;
  a.items = items; a.heads = c.heads; a.q_rows = Q; a.kv_len = kv; a.scale = 0.125f; a.nsplit = nsplit; a.part = part; a.lse = lse;
  return a;
}
// K/V of every cross layer in ONE GEMM: [items*kv, E] x [ncross*2*H, E]^T, scattered head-major.
int kv_project(const mra_qformer* h, const void* enc, int N, int kv, void* kv_cache, hipStream_t stream);
}  // namespace mra_host
