// The attached LM's entries of the C ABI (include/mra.h): argument checks, workspace layouts and launches.
//
// The reference wraps a causal LM around the Q-Formers' projections: LoRA adapters in its linears (models/xinstructblip.py:163), the
// cross-entropy of the answer tokens (:599-604), the prompt rows in front of it (:341-381, :541-595) and the greedy decode that picks
// the best checkpoint (self.llm_model.generate, :383-391).  The kernels behind those are lora.hip, lm_head.hip, prompt.hip, decode_attn.hip,
// prefill_attn.hip, prefill_attn_bwd.hip and lm_step.hip; this unit is the host code between the C entry and their launch functions (kernels.h).
//
// None of it has a handle: every entry takes device pointers, checks every argument before the first launch (a refused call writes nothing and
// leaves its reason in mra_last_error()), allocates nothing and enqueues on `stream`.  What the entries ask alike is asked once: lm_heads_check
// (operand type, head width, head grouping) by every attention-shaped entry, attn_call_check by mra_decode_attention,
// mra_prefill_attention and mra_prefill_attention_backward; DecodeWs is the one place the decode attention's workspace is laid out and carved, for the entry and for mra_lm_step.
#include <cmath>
#include <initializer_list>

#include "mra_handle.h"

using namespace mra;
using namespace mra_host;

extern "C" {

// ---- LoRA: the low-rank branch of an adapted linear of the attached LM (lora.hip) -------------------------------------------------------
// replaces: the peft LoraLayer branch of models/model_utils.py:4-14, applied at models/xinstructblip.py:163.  Every check comes before a launch.
namespace {

// the checks the three entries share; *thr = floor(p 2^32 + 0.5), the threshold the Python side computes the same way
int lora_check(const char* what, const void* t16, int64_t ld, int32_t rows, int32_t width, int32_t dtype, const void* a, const void* b, int32_t R,
               int32_t layout, double p, unsigned* thr) {
  const std::string w(what);
  if (rows < 0) return fail(MRA_EINVAL, w + ": negative rows");
  if (rows == 0) return MRA_OK;   // a no-op whatever else is passed (an empty tensor has no address)
  if (!t16 || !a || !b) return fail(MRA_EINVAL, w + ": null argument");
  if (dtype != MRA_F16 && dtype != MRA_BF16) return fail(MRA_EINVAL, w + ": dtype must be MRA_F16 or MRA_BF16");
  if (layout != MRA_LORA_NR && layout != MRA_LORA_RN) return fail(MRA_EINVAL, w + ": layout must be MRA_LORA_NR or MRA_LORA_RN");
  if (R < 1 || R > 16) return fail(MRA_EINVAL, w + ": R must be in 1..16");
  if (width <= 0 || width % 8) return fail(MRA_EINVAL, w + ": the width (K / N) must be a positive multiple of 8");
  if (ld < width) return fail(MRA_EINVAL, w + ": ld < width");
  if (ld % 8) return fail(MRA_EINVAL, w + ": the pitch must be a multiple of 8 elements (16 bytes)");
  if (!aligned16(t16) || !aligned16(a) || !aligned16(b)) return fail(MRA_EINVAL, w + ": pointers must be 16-byte aligned");
  if (!(p >= 0.0 && p < 1.0)) return fail(MRA_EINVAL, w + ": p must be in [0, 1)");
  const double t = std::floor(p * 4294967296.0 + 0.5);
  *thr = t >= 4294967295.0 ? 4294967295u : (unsigned)t;
  return MRA_OK;
}

}  // namespace

int mra_lora_down(const void* x, int64_t ldx, int32_t rows, int32_t K, int32_t dtype, const float* w, int32_t R, int32_t w_layout, float scale,
                  double p, uint64_t seed, float* out, void* stream) {
  unsigned thr = 0;
  if (int rc = lora_check("lora_down", x, ldx, rows, K, dtype, w, out, R, w_layout, p, &thr)) return rc;
  if (rows == 0) return MRA_OK;
  return chk(launch_lora_down(x, ldx, rows, K, w, R, w_layout, scale, thr, seed, out, dtype == MRA_BF16 ? OP_BF16 : OP_F16, as_stream(stream)),
             "lora_down");
}

int mra_lora_up_add(void* y, int64_t ldy, int32_t rows, int32_t N, int32_t dtype, const float* u, int32_t R, const float* w, int32_t w_layout,
                    float scale, double p, uint64_t seed, void* stream) {
  unsigned thr = 0;
  if (int rc = lora_check("lora_up_add", y, ldy, rows, N, dtype, u, w, R, w_layout, p, &thr)) return rc;
  if (rows == 0) return MRA_OK;
  return chk(launch_lora_up_add(y, ldy, rows, N, u, R, w, w_layout, scale, thr, seed, dtype == MRA_BF16 ? OP_BF16 : OP_F16, as_stream(stream)),
             "lora_up_add");
}

int mra_lora_wgrad(const void* x, int64_t ldx, int32_t rows, int32_t N, int32_t dtype, const float* u, int32_t R, float* dw, int32_t dw_layout,
                   float scale, double p, uint64_t seed, void* stream) {
  unsigned thr = 0;
  if (int rc = lora_check("lora_wgrad", x, ldx, rows, N, dtype, u, dw, R, dw_layout, p, &thr)) return rc;
  if (rows == 0) return MRA_OK;
  return chk(launch_lora_wgrad(x, ldx, rows, N, u, R, dw, dw_layout, scale, thr, seed, dtype == MRA_BF16 ? OP_BF16 : OP_F16, as_stream(stream)),
             "lora_wgrad");
}

// ---- the LM head + cross-entropy on the labelled rows (lm_head.hip) ----------------------------------------------------------------------
// replaces: lm_head + ForCausalLMLoss behind self.llm_model(..., labels=targets), models/xinstructblip.py:599-604.  Every check comes before a launch.
namespace {

// the workspace, in this order: tmax, tsum [R][tiles] f32 | zy [R] f32 | (want_grad) P~ [R][64 tiles] 16-bit | part [splits][R][K] f32
struct LmHeadWs {
  size_t stat, zy, p, part, total;
};
LmHeadWs lm_head_ws(int32_t R, int32_t V, int32_t K, int32_t want_grad) {
  LmHeadWs w{};
  const size_t nt = (size_t)lm_head_tiles(V);
  w.stat = up256(4 * (size_t)R * nt);
  w.zy = up256(4 * (size_t)R);
  w.p = want_grad ? up256(2 * (size_t)R * nt * LM_HEAD_TILE) : 0;
  w.part = want_grad ? up256(4 * (size_t)lm_head_splits(R, V, K) * (size_t)R * (size_t)K) : 0;
  w.total = 2 * w.stat + w.zy + w.p + w.part;
  return w;
}

int lm_head_check(const std::string& w, int32_t R, int32_t K, int32_t V, int32_t dtype, const void* x16, int64_t ldx, const char* xname,
                  const void* W, int64_t ldw, const void* labels, const void* a, const void* b, const void* workspace, size_t workspace_bytes, int32_t want_grad) {
  if (dtype != MRA_F16 && dtype != MRA_BF16) return fail(MRA_EINVAL, w + ": dtype must be MRA_F16 or MRA_BF16");
  if (V < 1) return fail(MRA_EINVAL, w + ": V must be at least 1");
  if (K <= 0 || K % 8) return fail(MRA_EINVAL, w + ": K must be a positive multiple of 8");
  if (!x16 || !W || !labels || !a || !b || !workspace) return fail(MRA_EINVAL, w + ": null argument");
  if (ldx < K) return fail(MRA_EINVAL, w + ": " + xname + " < K");
  if (ldw < K) return fail(MRA_EINVAL, w + ": ldw < K");
  if (ldx % 8 || ldw % 8) return fail(MRA_EINVAL, w + ": the pitches must be multiples of 8 elements (16 bytes)");
  if (!aligned16(x16) || !aligned16(W) || !aligned16(workspace)) return fail(MRA_EINVAL, w + ": h / dh, W and the workspace must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(labels) % 4 || reinterpret_cast<uintptr_t>(a) % 4 || reinterpret_cast<uintptr_t>(b) % 4)
    return fail(MRA_EINVAL, w + ": labels and the fp32 vectors must be 4-byte aligned");
  if (workspace_bytes < lm_head_ws(R, V, K, want_grad).total)
    return fail(MRA_EINVAL, w + ": workspace too small (mra_lm_head_ce_workspace_bytes)");
  return MRA_OK;
}

}  // namespace

size_t mra_lm_head_ce_workspace_bytes(int32_t R, int32_t V, int32_t K, int32_t dtype, int32_t want_grad) {
  if (R < 0 || V < 1 || K <= 0 || K % 8 || (dtype != MRA_F16 && dtype != MRA_BF16)) {
    fail(MRA_EINVAL, "lm_head_ce_workspace_bytes: R >= 0, V >= 1, K a positive multiple of 8, dtype MRA_F16 or MRA_BF16");
    return 0;
  }
  return lm_head_ws(R, V, K, want_grad != 0).total;
}

int mra_lm_head_ce_forward(const void* h, int64_t ldh, int32_t R, int32_t K, const void* W, int64_t ldw, int32_t V, int32_t dtype,
                           const int32_t* labels, float* nll, float* lse, void* workspace, size_t workspace_bytes, int32_t want_grad, void* stream) {
  const std::string w("lm_head_ce_forward");
  if (R < 0) return fail(MRA_EINVAL, w + ": negative R");
  if (R == 0) return MRA_OK;   // launches nothing, touches nothing
  if (int rc = lm_head_check(w, R, K, V, dtype, h, ldh, "ldh", W, ldw, labels, nll, lse, workspace, workspace_bytes, want_grad != 0)) return rc;
  const LmHeadWs ws = lm_head_ws(R, V, K, want_grad != 0);
  char* base = static_cast<char*>(workspace);
  float* tmax = reinterpret_cast<float*>(base);
  float* tsum = reinterpret_cast<float*>(base + ws.stat);
  float* zy = reinterpret_cast<float*>(base + 2 * ws.stat);
  void* P = want_grad ? base + 2 * ws.stat + ws.zy : nullptr;
  return chk(launch_lm_head_fwd(h, ldh, R, K, W, ldw, V, labels, nll, lse, tmax, tsum, zy, P, dtype == MRA_BF16 ? OP_BF16 : OP_F16, as_stream(stream)),
             "lm_head_ce_forward");
}

int mra_lm_head_ce_backward(const float* g, const void* W, int64_t ldw, int32_t V, int32_t K, int32_t dtype, const int32_t* labels, const float* lse,
                            void* workspace, size_t workspace_bytes, void* dh, int64_t lddh, int32_t R, void* stream) {
  const std::string w("lm_head_ce_backward");
  if (R < 0) return fail(MRA_EINVAL, w + ": negative R");
  if (R == 0) return MRA_OK;
  if (int rc = lm_head_check(w, R, K, V, dtype, dh, lddh, "lddh", W, ldw, labels, g, lse, workspace, workspace_bytes, 1)) return rc;
  const LmHeadWs ws = lm_head_ws(R, V, K, 1);
  char* base = static_cast<char*>(workspace);
  const float* tmax = reinterpret_cast<const float*>(base);
  const void* P = base + 2 * ws.stat + ws.zy;
  float* part = reinterpret_cast<float*>(base + 2 * ws.stat + ws.zy + ws.p);
  return chk(launch_lm_head_bwd(g, W, ldw, V, K, labels, lse, tmax, P, part, dh, lddh, R, dtype == MRA_BF16 ? OP_BF16 : OP_F16, as_stream(stream)),
             "lm_head_ce_backward");
}

// ---- what the attention-shaped entries ask alike -------------------------------------------------------------------------------------------
namespace {

// operand type, head width and head grouping: mra_decode_attention, mra_prefill_attention, mra_lm_step and the rotary debug entry
int lm_heads_check(const std::string& w, int32_t dtype, int32_t Hq, int32_t Hkv, int32_t D) {
  if (dtype != MRA_F16 && dtype != MRA_BF16) return fail(MRA_EINVAL, w + ": dtype must be MRA_F16 or MRA_BF16");
  if (D != 64 && D != 128) return fail(MRA_EINVAL, w + ": D must be 64 or 128");
  if (Hq < 1 || Hkv < 1 || Hq % Hkv) return fail(MRA_EINVAL, w + ": Hq must be a positive multiple of Hkv");
  const int G = Hq / Hkv;
  if (G != 1 && G != 2 && G != 4 && G != 8) return fail(MRA_EINVAL, w + ": Hq / Hkv must be 1, 2, 4 or 8");
  return MRA_OK;
}

// a q / k / v / out call with B >= 1: the heads, the grid limits, then `ptrs` (non-null, 16-byte aligned; `names`: how the entry lists them),
// `strides` (multiples of 8 elements), lse and scale
int attn_call_check(const std::string& w, int32_t B, int32_t dtype, int32_t Hq, int32_t Hkv, int32_t D, std::initializer_list<const void*> ptrs,
                    const char* names, std::initializer_list<int64_t> strides, const float* lse, float scale) {
  if (int rc = lm_heads_check(w, dtype, Hq, Hkv, D)) return rc;
  if (B > 65535 || Hkv > 65535) return fail(MRA_EINVAL, w + ": B and Hkv must be at most 65535");
  for (const void* p : ptrs)
    if (!p) return fail(MRA_EINVAL, w + ": null argument");
  for (const void* p : ptrs)
    if (!aligned16(p)) return fail(MRA_EINVAL, w + ": " + names + " must be 16-byte aligned");
  for (int64_t s : strides)
    if (s % 8) return fail(MRA_EINVAL, w + ": the strides must be multiples of 8 elements (16 bytes)");
  if (lse && !aligned4(lse)) return fail(MRA_EINVAL, w + ": lse must be 4-byte aligned");
  if (!std::isfinite(scale)) return fail(MRA_EINVAL, w + ": scale must be finite");
  return MRA_OK;
}

// the decode attention's workspace, in this order: chunk maxima, chunk sums [B][Hq][chunks] f32 | chunk accumulators [B][Hq][chunks][D] f32
struct DecodeWs {
  size_t stat, acc, total;
  void carve(void* base, DecodeArgs* a) const {
    char* b = static_cast<char*>(base);
    a->pm = reinterpret_cast<float*>(b);
    a->pl = reinterpret_cast<float*>(b + stat);
    a->pacc = reinterpret_cast<float*>(b + 2 * stat);
  }
};
DecodeWs decode_ws(int32_t B, int32_t Hq, int32_t S, int32_t D) {
  DecodeWs w{};
  const size_t rows = (size_t)B * (size_t)Hq * (size_t)decode_chunks(S);
  w.stat = up256(4 * rows);
  w.acc = up256(4 * rows * (size_t)D);
  w.total = 2 * w.stat + w.acc;
  return w;
}

}  // namespace

// ---- one-token attention of the LM's decode over a K/V cache read in place (decode_attn.hip) -----------------------------------------------
// replaces: scaled_dot_product_attention with one query row per head inside self.llm_model.generate(...), models/xinstructblip.py:383-391.
// Every check comes before a launch.
size_t mra_decode_attention_workspace_bytes(int32_t B, int32_t Hq, int32_t S, int32_t D) {
  if (B < 0 || Hq < 1 || S < 1 || (D != 64 && D != 128)) {
    fail(MRA_EINVAL, "decode_attention_workspace_bytes: B >= 0, Hq >= 1, S >= 1, D 64 or 128");
    return 0;
  }
  return decode_ws(B, Hq, S, D).total;
}

int mra_decode_attention(const void* q, int64_t q_sb, int64_t q_sh, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v,
                         int64_t v_sb, int64_t v_sh, int64_t v_ss, const uint8_t* mask, int64_t mask_sb, int32_t B, int32_t Hq, int32_t Hkv,
                         int32_t S, int32_t D, int32_t dtype, float scale, void* out, int64_t o_sb, int64_t o_sh, float* lse, void* workspace,
                         size_t workspace_bytes, void* stream) {
  const std::string w("decode_attention");
  if (B < 0) return fail(MRA_EINVAL, w + ": negative B");
  if (B == 0) return MRA_OK;   // launches nothing, touches nothing
  if (S < 1) return fail(MRA_EINVAL, w + ": S must be at least 1");
  if (int rc = attn_call_check(w, B, dtype, Hq, Hkv, D, {q, k, v, out, workspace}, "q, k, v, out and the workspace",
                               {q_sb, q_sh, k_sb, k_sh, k_ss, v_sb, v_sh, v_ss, o_sb, o_sh}, lse, scale))
    return rc;
  if (k_ss < D || v_ss < D) return fail(MRA_EINVAL, w + ": k_ss / v_ss < D");
  const DecodeWs ws = decode_ws(B, Hq, S, D);
  if (workspace_bytes < ws.total) return fail(MRA_EINVAL, w + ": workspace too small (mra_decode_attention_workspace_bytes)");
  DecodeArgs a{};
  a.q = q; a.q_sb = q_sb; a.q_sh = q_sh;
  a.k = k; a.k_sb = k_sb; a.k_sh = k_sh; a.k_ss = k_ss;
  a.v = v; a.v_sb = v_sb; a.v_sh = v_sh; a.v_ss = v_ss;
  a.mask = mask; a.mask_sb = mask_sb;
  a.B = B; a.Hq = Hq; a.Hkv = Hkv; a.S = S;
  a.scale = scale;
  a.out = out; a.o_sb = o_sb; a.o_sh = o_sh;
  a.lse = lse;
  ws.carve(workspace, &a);
  return chk(launch_decode_attention(a, D, dtype == MRA_BF16 ? OP_BF16 : OP_F16, as_stream(stream)), "decode_attention");
}

// ---- causal grouped-query attention of the LM's prefill (prefill_attn.hip) ----------------------------------------------------------------
// replaces: scaled_dot_product_attention under the [Sq][Skv] mask in the prefill inside self.llm_model.generate(...),
// models/xinstructblip.py:388-391.  Every check comes before the launch.
int mra_prefill_attention(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                          const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, const uint8_t* mask, int64_t mask_sb, int32_t B, int32_t Hq,
                          int32_t Hkv, int32_t Sq, int32_t Skv, int32_t q_offset, int32_t D, int32_t dtype, float scale, void* out, int64_t o_sb,
                          int64_t o_ss, int64_t o_sh, float* lse, void* stream) {
  const std::string w("prefill_attention");
  if (B < 0) return fail(MRA_EINVAL, w + ": negative B");
  if (B == 0) return MRA_OK;   // launches nothing, touches nothing
  if (Sq < 1 || Skv < 1) return fail(MRA_EINVAL, w + ": Sq and Skv must be at least 1");
  if (q_offset < 0 || (int64_t)q_offset + Sq > Skv) return fail(MRA_EINVAL, w + ": 0 <= q_offset and q_offset + Sq <= Skv expected");
  if (Skv > PREFILL_MAX_SKV || prefill_qblocks(Sq) > 65535) return fail(MRA_EINVAL, w + ": Skv must be at most 2^30 and Sq at most 65535 query blocks");
  if (int rc = attn_call_check(w, B, dtype, Hq, Hkv, D, {q, k, v, out}, "q, k, v and out",
                               {q_sb, q_sh, q_ss, k_sb, k_sh, k_ss, v_sb, v_sh, v_ss, o_sb, o_ss, o_sh}, lse, scale))
    return rc;
  if (q_ss < D || k_ss < D || v_ss < D || o_ss < D || o_sh < D) return fail(MRA_EINVAL, w + ": a position stride (or out's head stride) below D");
  PrefillArgs a{};
  a.q = q; a.q_sb = q_sb; a.q_sh = q_sh; a.q_ss = q_ss;
  a.k = k; a.k_sb = k_sb; a.k_sh = k_sh; a.k_ss = k_ss;
  a.v = v; a.v_sb = v_sb; a.v_sh = v_sh; a.v_ss = v_ss;
  a.mask = mask; a.mask_sb = mask_sb;
  a.B = B; a.Hq = Hq; a.G = Hq / Hkv; a.Sq = Sq; a.Skv = Skv; a.q_offset = q_offset;
  a.scale = scale;
  a.out = out; a.o_sb = o_sb; a.o_ss = o_ss; a.o_sh = o_sh;
  a.lse = lse;
  return chk(launch_prefill_attention(a, D, dtype == MRA_BF16 ? OP_BF16 : OP_F16, as_stream(stream)), "prefill_attention");
}

// ---- its backward: dQ, dK, dV of the causal grouped-query attention in training (prefill_attn_bwd.hip) ------------------------------------
// replaces: the backward of scaled_dot_product_attention under the [S][S] mask inside self.llm_model(inputs_embeds=..., labels=...),
// models/xinstructblip.py:599-604.  Every check comes before a launch.  The workspace is delta, f32 [B][Hq][Sq].
size_t mra_prefill_attention_backward_workspace_bytes(int32_t B, int32_t Hq, int32_t Sq) {
  if (B < 0 || Hq < 1 || Sq < 1) {
    fail(MRA_EINVAL, "prefill_attention_backward_workspace_bytes: B >= 0, Hq >= 1, Sq >= 1");
    return 0;
  }
  return up256(4 * (size_t)B * (size_t)Hq * (size_t)Sq);
}

int mra_prefill_attention_backward(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                                   const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, const uint8_t* mask, int64_t mask_sb, const void* out,
                                   int64_t o_sb, int64_t o_ss, int64_t o_sh, const void* dout, int64_t do_sb, int64_t do_ss, int64_t do_sh,
                                   const float* lse, int32_t B, int32_t Hq, int32_t Hkv, int32_t Sq, int32_t Skv, int32_t q_offset, int32_t D,
                                   int32_t dtype, float scale, void* dq, int64_t dq_sb, int64_t dq_sh, int64_t dq_ss, void* dk, int64_t dk_sb,
                                   int64_t dk_sh, int64_t dk_ss, void* dv, int64_t dv_sb, int64_t dv_sh, int64_t dv_ss, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  const std::string w("prefill_attention_backward");
  if (B < 0) return fail(MRA_EINVAL, w + ": negative B");
  if (B == 0) return MRA_OK;   // launches nothing, touches nothing
  if (Sq < 1 || Skv < 1) return fail(MRA_EINVAL, w + ": Sq and Skv must be at least 1");
  if (q_offset < 0 || (int64_t)q_offset + Sq > Skv) return fail(MRA_EINVAL, w + ": 0 <= q_offset and q_offset + Sq <= Skv expected");
  if (Skv > 65535 * PREFILL_BWD_KB) return fail(MRA_EINVAL, w + ": Skv must be at most 65535 key blocks");
  if (!lse) return fail(MRA_EINVAL, w + ": null argument (lse is mandatory)");
  if (int rc = attn_call_check(w, B, dtype, Hq, Hkv, D, {q, k, v, out, dout, dq, dk, dv, workspace}, "q, k, v, out, dout, dq, dk, dv and the workspace",
                               {q_sb, q_sh, q_ss, k_sb, k_sh, k_ss, v_sb, v_sh, v_ss, o_sb, o_ss, o_sh, do_sb, do_ss, do_sh, dq_sb, dq_sh, dq_ss,
                                dk_sb, dk_sh, dk_ss, dv_sb, dv_sh, dv_ss},
                               lse, scale))
    return rc;
  if (q_ss < D || k_ss < D || v_ss < D || o_ss < D || o_sh < D || do_ss < D || do_sh < D || dq_ss < D || dk_ss < D || dv_ss < D)
    return fail(MRA_EINVAL, w + ": a position stride (or out's / dout's head stride) below D");
  if (workspace_bytes < up256(4 * (size_t)B * (size_t)Hq * (size_t)Sq))
    return fail(MRA_EINVAL, w + ": workspace too small (mra_prefill_attention_backward_workspace_bytes)");
  PrefillBwdArgs a{};
  a.q = q; a.q_sb = q_sb; a.q_sh = q_sh; a.q_ss = q_ss;
  a.k = k; a.k_sb = k_sb; a.k_sh = k_sh; a.k_ss = k_ss;
  a.v = v; a.v_sb = v_sb; a.v_sh = v_sh; a.v_ss = v_ss;
  a.mask = mask; a.mask_sb = mask_sb;
  a.out = out; a.o_sb = o_sb; a.o_ss = o_ss; a.o_sh = o_sh;
  a.dout = dout; a.do_sb = do_sb; a.do_ss = do_ss; a.do_sh = do_sh;
  a.lse = lse;
  a.B = B; a.Hq = Hq; a.G = Hq / Hkv; a.Sq = Sq; a.Skv = Skv; a.q_offset = q_offset;
  a.scale = scale;
  a.dq = dq; a.dq_sb = dq_sb; a.dq_sh = dq_sh; a.dq_ss = dq_ss;
  a.dk = dk; a.dk_sb = dk_sb; a.dk_sh = dk_sh; a.dk_ss = dk_ss;
  a.dv = dv; a.dv_sb = dv_sb; a.dv_sh = dv_sh; a.dv_ss = dv_ss;
  a.delta = static_cast<float*>(workspace);
  return chk(launch_prefill_attention_backward(a, D, dtype == MRA_BF16 ? OP_BF16 : OP_F16, as_stream(stream)), "prefill_attention_backward");
}

// ---- one whole token of the LM's decode (lm_step.hip) ---------------------------------------------------------------------------------------
// replaces: one iteration of self.llm_model.generate(...) behind the prefill, models/xinstructblip.py:383-391.  Every check comes before a launch.
namespace {

struct LmStepWs {
  size_t xn, u, q, act, attn, total;
};
LmStepWs lm_step_ws(int32_t B, int32_t hidden, int32_t inter, int32_t Hq, int32_t D, int32_t Smax) {
  LmStepWs w{};
  w.xn = up256(4 * (size_t)B * (size_t)hidden);
  w.u = up256(4 * (size_t)B * LM_MAX_R);
  w.q = up256(2 * (size_t)B * (size_t)Hq * (size_t)D);
  w.act = up256(2 * (size_t)B * (size_t)inter);
  w.attn = decode_ws(B, Hq, Smax, D).total;
  w.total = w.xn + 3 * w.u + 2 * w.q + w.act + w.attn;
  return w;
}

// one linear of a step or of the debug entry: pointers, pitch, adapter
int lm_linear_check(const std::string& w, const mra_lm_linear& l, int32_t N, int32_t K) {
  if (!l.W) return fail(MRA_EINVAL, w + ": null W");
  if (!aligned16(l.W)) return fail(MRA_EINVAL, w + ": W must be 16-byte aligned");
  if (l.N != N || N < 1) return fail(MRA_EINVAL, w + ": N is not the layer's");
  if (l.ldw < K || l.ldw % 8) return fail(MRA_EINVAL, w + ": ldw must be at least K and a multiple of 8 elements");
  if (l.R < 0 || l.R > LM_MAX_R) return fail(MRA_EINVAL, w + ": R must be in 0..16");
  if (l.R > 0) {
    if (!l.A || !l.Bw) return fail(MRA_EINVAL, w + ": null adapter");
    if (!aligned16(l.A) || !aligned4(l.Bw)) return fail(MRA_EINVAL, w + ": the adapters must be aligned (A 16 bytes, Bw 4)");
    if (!std::isfinite(l.scale)) return fail(MRA_EINVAL, w + ": scale must be finite");
  }
  return MRA_OK;
}

LmSeg lm_seg(const mra_lm_linear& l, const float* u, void* out, long long ldo) {
  LmSeg s{};
  s.W = l.W; s.ldw = l.ldw; s.N = l.N; s.R = l.R; s.Bw = l.Bw; s.u = u; s.scale = l.scale; s.out = out; s.ldo = ldo;
  return s;
}

int lm_dims_check(const std::string& w, int32_t B, int32_t dtype, int32_t Hq, int32_t Hkv, int32_t D) {
  if (B < 1 || B > LM_MAX_B) return fail(MRA_EINVAL, w + ": B must be in 1..8");
  return lm_heads_check(w, dtype, Hq, Hkv, D);
}

}  // namespace

size_t mra_lm_step_workspace_bytes(int32_t B, int32_t hidden, int32_t intermediate, int32_t Hq, int32_t D, int32_t Smax) {
  if (B < 1 || B > LM_MAX_B || hidden < 8 || hidden % 8 || intermediate < 8 || intermediate % 8 || Hq < 1 || (D != 64 && D != 128) || Smax < 1) {
    fail(MRA_EINVAL, "lm_step_workspace_bytes: B in 1..8, hidden and intermediate positive multiples of 8, Hq >= 1, D 64 or 128, Smax >= 1");
    return 0;
  }
  return lm_step_ws(B, hidden, intermediate, Hq, D, Smax).total;
}

int mra_lm_step(const mra_lm_step_desc* d, void* stream) {
  const std::string w("lm_step");
  if (!d) return fail(MRA_EINVAL, w + ": null descriptor");
  if (d->struct_bytes != sizeof(mra_lm_step_desc)) return fail(MRA_EINVAL, w + ": struct_bytes is not sizeof(mra_lm_step_desc)");
  if (int rc = lm_dims_check(w, d->B, d->dtype, d->Hq, d->Hkv, d->D)) return rc;
  const int B = d->B, H = d->hidden, I = d->intermediate, Hq = d->Hq, Hkv = d->Hkv, D = d->D;
  if (H < 8 || H % 8 || I < 8 || I % 8) return fail(MRA_EINVAL, w + ": hidden and intermediate (K) must be positive multiples of 8");
  if (d->L < 1 || d->V < 1) return fail(MRA_EINVAL, w + ": L and V must be at least 1");
  if (!std::isfinite(d->eps) || !std::isfinite(d->attn_scale)) return fail(MRA_EINVAL, w + ": eps and attn_scale must be finite");
  if (d->Smax < 1 || d->slot < 0 || d->slot >= d->Smax) return fail(MRA_EINVAL, w + ": slot must be in [0, Smax)");
  if (d->n_eos < 0 || d->n_eos > LM_MAX_EOS) return fail(MRA_EINVAL, w + ": n_eos must be in 0..8");
  if (!d->layers || !d->final_norm || !d->head || !d->mask || !d->position || !d->cos || !d->sin || !d->h || !d->logits || !d->tokens_out || !d->workspace)
    return fail(MRA_EINVAL, w + ": null argument");
  if (d->tokens_in && !d->embed) return fail(MRA_EINVAL, w + ": tokens_in without an embedding table");
  if (!aligned16(d->final_norm) || !aligned16(d->head) || !aligned16(d->h) || !aligned16(d->workspace) || !aligned16(d->cos) || !aligned16(d->sin) ||
      !aligned16(d->logits) || (d->embed && !aligned16(d->embed)))
    return fail(MRA_EINVAL, w + ": embed, final_norm, head, h, logits, cos, sin and the workspace must be 16-byte aligned");
  if (!aligned4(d->position) || !aligned4(d->tokens_in) || !aligned4(d->tokens_out) || !aligned4(d->finished))
    return fail(MRA_EINVAL, w + ": position, tokens and finished must be 4-byte aligned");
  if (d->ld_head < H || d->ld_head % 8 || (d->embed && (d->ld_embed < H || d->ld_embed % 8)))
    return fail(MRA_EINVAL, w + ": ld_head / ld_embed must be at least hidden and multiples of 8 elements");
  if (d->ld_logits < d->V) return fail(MRA_EINVAL, w + ": ld_logits < V");
  if (d->rope_ld < D || d->rope_rows < 1) return fail(MRA_EINVAL, w + ": the rotary table needs rope_rows >= 1 rows of rope_ld >= D values");
  if (d->k_sb % 8 || d->k_sh % 8 || d->k_ss % 8 || d->v_sb % 8 || d->v_sh % 8 || d->v_ss % 8)
    return fail(MRA_EINVAL, w + ": the cache strides must be multiples of 8 elements (16 bytes)");
  if (d->k_ss < D || d->v_ss < D) return fail(MRA_EINVAL, w + ": k_ss / v_ss < D");
  if (d->mask_sb < (int64_t)d->slot + 1 && B > 1) return fail(MRA_EINVAL, w + ": mask_sb < slot + 1");
  for (int l = 0; l < d->L; ++l) {
    const mra_lm_layer& y = d->layers[l];
    const std::string wl = w + ": layer " + std::to_string(l);
    if (!y.norm1 || !y.norm2 || !y.kcache || !y.vcache) return fail(MRA_EINVAL, wl + ": null argument");
    if (!aligned16(y.norm1) || !aligned16(y.norm2) || !aligned16(y.kcache) || !aligned16(y.vcache))
      return fail(MRA_EINVAL, wl + ": the gains and the caches must be 16-byte aligned");
    if (int rc = lm_linear_check(wl + " q", y.q, Hq * D, H)) return rc;
    if (int rc = lm_linear_check(wl + " k", y.k, Hkv * D, H)) return rc;
    if (int rc = lm_linear_check(wl + " v", y.v, Hkv * D, H)) return rc;
    if (int rc = lm_linear_check(wl + " o", y.o, H, Hq * D)) return rc;
    if (int rc = lm_linear_check(wl + " gate", y.gate, I, H)) return rc;
    if (int rc = lm_linear_check(wl + " up", y.up, I, H)) return rc;
    if (int rc = lm_linear_check(wl + " down", y.down, H, I)) return rc;
  }
  const LmStepWs ws = lm_step_ws(B, H, I, Hq, D, d->Smax);
  if (d->workspace_bytes < ws.total) return fail(MRA_EINVAL, w + ": workspace too small (mra_lm_step_workspace_bytes)");

  char* base = static_cast<char*>(d->workspace);
  float* xn = reinterpret_cast<float*>(base);
  float* u[3] = {reinterpret_cast<float*>(base + ws.xn), reinterpret_cast<float*>(base + ws.xn + ws.u), reinterpret_cast<float*>(base + ws.xn + 2 * ws.u)};
  void* q = base + ws.xn + 3 * ws.u;
  void* ao = base + ws.xn + 3 * ws.u + ws.q;
  void* act = base + ws.xn + 3 * ws.u + 2 * ws.q;
  const int op = d->dtype == MRA_BF16 ? OP_BF16 : OP_F16;
  hipStream_t st = as_stream(stream);
  DecodeArgs at{};   // every layer's attention over the slots 0 .. slot; k and v are set per layer
  at.q = q; at.q_sb = (long long)Hq * D; at.q_sh = D;
  at.k_sb = d->k_sb; at.k_sh = d->k_sh; at.k_ss = d->k_ss;
  at.v_sb = d->v_sb; at.v_sh = d->v_sh; at.v_ss = d->v_ss;
  at.mask = d->mask; at.mask_sb = d->mask_sb;
  at.B = B; at.Hq = Hq; at.Hkv = Hkv; at.S = d->slot + 1;
  at.scale = d->attn_scale;
  at.out = ao; at.o_sb = (long long)Hq * D; at.o_sh = D;
  decode_ws(B, Hq, at.S, D).carve(base + ws.xn + 3 * ws.u + 2 * ws.q + ws.act, &at);

  auto prep = [&](const void* x, int K, const void* gain, const mra_lm_linear* a0, const mra_lm_linear* a1, const mra_lm_linear* a2) {
    LmPrep p{};
    p.B = B; p.K = K; p.x = x; p.ldx = K; p.gain = gain; p.eps = d->eps; p.xn = xn;
    const mra_lm_linear* as[3] = {a0, a1, a2};
    for (int a = 0; a < 3; ++a) {
      p.A[a] = as[a] ? as[a]->A : nullptr;
      p.R[a] = as[a] ? as[a]->R : 0;
      p.u[a] = u[a];
    }
    return launch_lm_prep(p, op, st);
  };
  auto skinny = [&](int epi, const void* x, int x_f32, int K) {
    LmSkinny p{};
    p.B = B; p.K = K; p.epi = epi; p.x = x; p.x_f32 = x_f32; p.ldx = K;
    return p;
  };
#define MRA_LM_DO(call)                       \
  if (int rc = (call)) return chk(rc, "lm_step")
  if (d->tokens_in) MRA_LM_DO(launch_lm_embed(d->tokens_in, d->embed, d->ld_embed, d->V, B, H, d->h, H, op, st));
  for (int l = 0; l < d->L; ++l) {
    const mra_lm_layer& y = d->layers[l];
    MRA_LM_DO(prep(d->h, H, y.norm1, &y.q, &y.k, &y.v));
    {
      LmSkinny p = skinny(LM_EPI_ROPE, xn, 1, H);
      p.nseg = 3;
      p.seg[0] = lm_seg(y.q, u[0], q, (long long)Hq * D);
      p.seg[1] = lm_seg(y.k, u[1], nullptr, 0);
      p.seg[2] = lm_seg(y.v, u[2], nullptr, 0);
      p.Hq = Hq; p.Hkv = Hkv; p.D = D; p.slot = d->slot; p.pos_offset = d->pos_offset; p.rope_rows = d->rope_rows;
      p.position = d->position; p.cos = d->cos; p.sin = d->sin; p.rope_ld = d->rope_ld;
      p.kc = y.kcache; p.vc = y.vcache;
      p.k_sb = d->k_sb; p.k_sh = d->k_sh; p.k_ss = d->k_ss; p.v_sb = d->v_sb; p.v_sh = d->v_sh; p.v_ss = d->v_ss;
      MRA_LM_DO(launch_lm_skinny(p, op, st));
    }
    at.k = y.kcache; at.v = y.vcache;
    MRA_LM_DO(launch_decode_attention(at, D, op, st));
    if (y.o.R > 0) MRA_LM_DO(prep(ao, Hq * D, nullptr, &y.o, nullptr, nullptr));
    {
      LmSkinny p = skinny(LM_EPI_RES, ao, 0, Hq * D);
      p.nseg = 1;
      p.seg[0] = lm_seg(y.o, u[0], d->h, H);
      p.res = d->h; p.ldres = H;
      MRA_LM_DO(launch_lm_skinny(p, op, st));
    }
    MRA_LM_DO(prep(d->h, H, y.norm2, &y.gate, &y.up, nullptr));
    {
      LmSkinny p = skinny(LM_EPI_SWIGLU, xn, 1, H);
      p.nseg = 2;
      p.seg[0] = lm_seg(y.gate, u[0], act, I);
      p.seg[1] = lm_seg(y.up, u[1], nullptr, 0);
      MRA_LM_DO(launch_lm_skinny(p, op, st));
    }
    if (y.down.R > 0) MRA_LM_DO(prep(act, I, nullptr, &y.down, nullptr, nullptr));
    {
      LmSkinny p = skinny(LM_EPI_RES, act, 0, I);
      p.nseg = 1;
      p.seg[0] = lm_seg(y.down, u[0], d->h, H);
      p.res = d->h; p.ldres = H;
      MRA_LM_DO(launch_lm_skinny(p, op, st));
    }
  }
  MRA_LM_DO(prep(d->h, H, d->final_norm, nullptr, nullptr, nullptr));
  {
    LmSkinny p = skinny(LM_EPI_PLAIN, xn, 1, H);
    p.nseg = 1;
    p.out_f32 = 1;
    mra_lm_linear head{};
    head.W = d->head; head.ldw = d->ld_head; head.N = d->V;
    p.seg[0] = lm_seg(head, nullptr, d->logits, d->ld_logits);
    MRA_LM_DO(launch_lm_skinny(p, op, st));
  }
  LmGreedy g{};
  g.tokens_out = d->tokens_out; g.finished = d->finished; g.pad = d->pad; g.n_eos = d->n_eos;
  for (int e = 0; e < d->n_eos; ++e) g.eos[e] = d->eos[e];
  MRA_LM_DO(launch_lm_argmax(d->logits, d->ld_logits, B, d->V, g, st));
#undef MRA_LM_DO
  return MRA_OK;
}

int mra_debug_lm_skinny(const mra_lm_skinny_desc* d, void* stream) {
  const std::string w("debug_lm_skinny");
  if (!d) return fail(MRA_EINVAL, w + ": null descriptor");
  if (d->struct_bytes != sizeof(mra_lm_skinny_desc)) return fail(MRA_EINVAL, w + ": struct_bytes is not sizeof(mra_lm_skinny_desc)");
  const int epi = d->epilogue, B = d->B, K = d->K;
  if (epi < LM_EPI_PLAIN || epi > LM_EPI_ROPE) return fail(MRA_EINVAL, w + ": epilogue must be 0 .. 3");
  if (B < 1 || B > LM_MAX_B) return fail(MRA_EINVAL, w + ": B must be in 1..8");
  if (d->dtype != MRA_F16 && d->dtype != MRA_BF16) return fail(MRA_EINVAL, w + ": dtype must be MRA_F16 or MRA_BF16");
  if (K < 8 || K % 8) return fail(MRA_EINVAL, w + ": K must be a positive multiple of 8");
  if (d->nseg < 1 || d->nseg > 3) return fail(MRA_EINVAL, w + ": nseg must be in 1..3");
  if (epi == LM_EPI_SWIGLU && (d->nseg != 2 || d->seg[0].N != d->seg[1].N)) return fail(MRA_EINVAL, w + ": SwiGLU takes two segments of one N");
  if (epi == LM_EPI_ROPE) {
    if (int rc = lm_dims_check(w, B, d->dtype, d->Hq, d->Hkv, d->D)) return rc;
    if (d->nseg != 3 || d->seg[0].N != d->Hq * d->D || d->seg[1].N != d->Hkv * d->D || d->seg[2].N != d->Hkv * d->D)
      return fail(MRA_EINVAL, w + ": the rotary form takes q, k, v with N = Hq D, Hkv D, Hkv D");
  }
  if (d->out_f32 && epi != LM_EPI_PLAIN) return fail(MRA_EINVAL, w + ": fp32 output belongs to the plain epilogue");
  if (!d->x || !aligned16(d->x)) return fail(MRA_EINVAL, w + ": x must be non-null and 16-byte aligned");
  if (d->ldx < K || d->ldx % 8) return fail(MRA_EINVAL, w + ": ldx must be at least K and a multiple of 8 elements");
  if (d->x_bytes < 2 * ((uint64_t)(B - 1) * (uint64_t)d->ldx + (uint64_t)K)) return fail(MRA_EINVAL, w + ": x footprint beyond x_bytes");
  if (d->norm_gain && !aligned16(d->norm_gain)) return fail(MRA_EINVAL, w + ": norm_gain must be 16-byte aligned");
  if (!std::isfinite(d->eps)) return fail(MRA_EINVAL, w + ": eps must be finite");
  bool need_prep = d->norm_gain != nullptr;
  const size_t out_es = d->out_f32 ? 4 : 2;
  for (int s = 0; s < d->nseg; ++s) {
    const std::string wsn = w + ": segment " + std::to_string(s);
    if (int rc = lm_linear_check(wsn, d->seg[s], d->seg[s].N, K)) return rc;
    if (d->w_bytes[s] < 2 * ((uint64_t)(d->seg[s].N - 1) * (uint64_t)d->seg[s].ldw + (uint64_t)K)) return fail(MRA_EINVAL, wsn + ": W footprint beyond w_bytes");
    need_prep = need_prep || d->seg[s].R > 0;
    const bool has_out = epi == LM_EPI_PLAIN || epi == LM_EPI_RES || s == 0;
    if (has_out) {
      if (!d->out[s] || !aligned16(d->out[s])) return fail(MRA_EINVAL, wsn + ": out must be non-null and 16-byte aligned");
      if (d->ldo[s] < d->seg[s].N || (!d->out_f32 && d->ldo[s] % 8)) return fail(MRA_EINVAL, wsn + ": ldo must be at least N and a multiple of 8 elements");
      if (d->out_bytes[s] < out_es * ((uint64_t)(B - 1) * (uint64_t)d->ldo[s] + (uint64_t)d->seg[s].N)) return fail(MRA_EINVAL, wsn + ": out footprint beyond out_bytes");
    }
  }
  if (epi == LM_EPI_RES) {
    if (d->nseg != 1) return fail(MRA_EINVAL, w + ": the residual epilogue takes one segment");
    if (!d->res || !aligned16(d->res)) return fail(MRA_EINVAL, w + ": res must be non-null and 16-byte aligned");
    if (d->ldres < d->seg[0].N || d->ldres % 8) return fail(MRA_EINVAL, w + ": ldres must be at least N and a multiple of 8 elements");
    if (d->res_bytes < 2 * ((uint64_t)(B - 1) * (uint64_t)d->ldres + (uint64_t)d->seg[0].N)) return fail(MRA_EINVAL, w + ": res footprint beyond res_bytes");
  }
  if (epi == LM_EPI_ROPE) {
    if (!d->position || !d->cos || !d->sin || !d->kcache || !d->vcache) return fail(MRA_EINVAL, w + ": null rotary / cache argument");
    if (!aligned4(d->position) || !aligned16(d->cos) || !aligned16(d->sin) || !aligned16(d->kcache) || !aligned16(d->vcache))
      return fail(MRA_EINVAL, w + ": position (4), cos, sin and the caches (16) must be aligned");
    if (d->rope_rows < 1 || d->rope_ld < d->D) return fail(MRA_EINVAL, w + ": the rotary table needs rope_rows >= 1 rows of rope_ld >= D values");
    if (d->rope_bytes < 4 * ((uint64_t)(d->rope_rows - 1) * (uint64_t)d->rope_ld + (uint64_t)d->D)) return fail(MRA_EINVAL, w + ": rotary footprint beyond rope_bytes");
    if (d->slot < 0) return fail(MRA_EINVAL, w + ": negative slot");
    if (d->k_sb % 8 || d->k_sh % 8 || d->k_ss % 8 || d->v_sb % 8 || d->v_sh % 8 || d->v_ss % 8 || d->k_sb < 0 || d->k_sh < 0 || d->v_sb < 0 || d->v_sh < 0)
      return fail(MRA_EINVAL, w + ": the cache strides must be non-negative multiples of 8 elements (16 bytes)");
    if (d->k_ss < d->D || d->v_ss < d->D) return fail(MRA_EINVAL, w + ": k_ss / v_ss < D");
    const uint64_t kf = (uint64_t)(B - 1) * d->k_sb + (uint64_t)(d->Hkv - 1) * d->k_sh + (uint64_t)d->slot * d->k_ss + d->D;
    const uint64_t vf = (uint64_t)(B - 1) * d->v_sb + (uint64_t)(d->Hkv - 1) * d->v_sh + (uint64_t)d->slot * d->v_ss + d->D;
    if (d->kcache_bytes < 2 * kf || d->vcache_bytes < 2 * vf) return fail(MRA_EINVAL, w + ": slot beyond the cache (footprint beyond kcache_bytes / vcache_bytes)");
  }
  const size_t xn_b = up256(4 * (size_t)B * (size_t)K), u_b = up256(4 * (size_t)B * LM_MAX_R);
  if (need_prep) {
    if (!d->workspace || !aligned16(d->workspace)) return fail(MRA_EINVAL, w + ": workspace must be non-null and 16-byte aligned");
    if (d->workspace_bytes < xn_b + 3 * u_b) return fail(MRA_EINVAL, w + ": workspace too small");
  }
  char* base = static_cast<char*>(d->workspace);
  float* xn = reinterpret_cast<float*>(base);
  const int op = d->dtype == MRA_BF16 ? OP_BF16 : OP_F16;
  LmSkinny p{};
  p.B = B; p.K = K; p.nseg = d->nseg; p.epi = epi; p.out_f32 = d->out_f32;
  p.x = d->norm_gain ? (const void*)xn : d->x;
  p.x_f32 = d->norm_gain ? 1 : 0;
  p.ldx = d->norm_gain ? K : d->ldx;
  LmPrep pp{};
  pp.B = B; pp.K = K; pp.x = d->x; pp.ldx = d->ldx; pp.gain = d->norm_gain; pp.eps = d->eps; pp.xn = xn;
  for (int s = 0; s < d->nseg; ++s) {
    float* u = need_prep ? reinterpret_cast<float*>(base + xn_b + s * u_b) : nullptr;
    pp.A[s] = d->seg[s].A; pp.R[s] = d->seg[s].R; pp.u[s] = u;
    p.seg[s] = lm_seg(d->seg[s], u, d->out[s], d->ldo[s]);
  }
  p.res = d->res; p.ldres = d->ldres;
  p.Hq = d->Hq; p.Hkv = d->Hkv; p.D = d->D; p.slot = d->slot; p.pos_offset = d->pos_offset; p.rope_rows = d->rope_rows;
  p.position = d->position; p.cos = d->cos; p.sin = d->sin; p.rope_ld = d->rope_ld;
  p.kc = d->kcache; p.vc = d->vcache;
  p.k_sb = d->k_sb; p.k_sh = d->k_sh; p.k_ss = d->k_ss; p.v_sb = d->v_sb; p.v_sh = d->v_sh; p.v_ss = d->v_ss;
  if (need_prep)
    if (int rc = launch_lm_prep(pp, op, as_stream(stream))) return chk(rc, "debug_lm_skinny (prologue)");
  return chk(launch_lm_skinny(p, op, as_stream(stream)), "debug_lm_skinny");
}

int mra_debug_lm_argmax(const float* logits, int64_t ld, int32_t B, int32_t V, int32_t* tokens_out, int32_t* finished, int32_t pad,
                        const int32_t* eos, int32_t n_eos, void* stream) {
  const std::string w("debug_lm_argmax");
  if (B < 1 || V < 1 || ld < V) return fail(MRA_EINVAL, w + ": B >= 1, V >= 1 and ld >= V expected");
  if (n_eos < 0 || n_eos > LM_MAX_EOS || (n_eos > 0 && !eos)) return fail(MRA_EINVAL, w + ": n_eos must be in 0..8 (with a host array)");
  if (!logits || !tokens_out) return fail(MRA_EINVAL, w + ": null argument");
  if (!aligned4(logits) || !aligned4(tokens_out) || !aligned4(finished)) return fail(MRA_EINVAL, w + ": buffers must be 4-byte aligned");
  LmGreedy g{};
  g.tokens_out = tokens_out; g.finished = finished; g.pad = pad; g.n_eos = n_eos;
  for (int e = 0; e < n_eos; ++e) g.eos[e] = eos[e];
  return chk(launch_lm_argmax(logits, ld, B, V, g, as_stream(stream)), "debug_lm_argmax");
}

// ---- prompt assembly: one row gather with a cast (prompt.hip) -----------------------------------------------------------------------------
// replaces: the torch.cat in front of the LM, models/xinstructblip.py:341-381, :541-595.  Every check comes before a launch.
int mra_gather_rows(void* out, int64_t ldo, int32_t out_dtype, int32_t n_rows, int32_t width, const mra_rows_src* srcs, int32_t n_src,
                    const int32_t* plan, void* stream) {
  const std::string w("gather_rows");
  if (n_rows < 0) return fail(MRA_EINVAL, w + ": negative n_rows");
  if (n_rows == 0) return MRA_OK;   // launches nothing, touches nothing
  if (!out || !srcs || !plan) return fail(MRA_EINVAL, w + ": null argument");
  if (n_src < 1 || n_src > GATHER_MAX_SRC) return fail(MRA_EINVAL, w + ": n_src must be in 1..4");
  if (width <= 0 || width % 8) return fail(MRA_EINVAL, w + ": width must be a positive multiple of 8");
  if (out_dtype != MRA_F32 && out_dtype != MRA_F16 && out_dtype != MRA_BF16) return fail(MRA_EINVAL, w + ": unknown out_dtype");
  if (ldo < width) return fail(MRA_EINVAL, w + ": ldo < width");
  if (ldo % (out_dtype == MRA_F32 ? 4 : 8)) return fail(MRA_EINVAL, w + ": the output pitch must be a multiple of 16 bytes");
  if (!aligned16(out)) return fail(MRA_EINVAL, w + ": out must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(plan) % 8) return fail(MRA_EINVAL, w + ": plan must be 8-byte aligned");
  const void* ptrs[GATHER_MAX_SRC];
  long long lds[GATHER_MAX_SRC];
  int rows[GATHER_MAX_SRC], dts[GATHER_MAX_SRC];
  for (int k = 0; k < n_src; ++k) {
    const mra_rows_src& s = srcs[k];
    const std::string sk = w + ": source " + std::to_string(k);
    if (!s.ptr) return fail(MRA_EINVAL, sk + ": null ptr");
    if (s.dtype != MRA_F32 && s.dtype != MRA_F16 && s.dtype != MRA_BF16) return fail(MRA_EINVAL, sk + ": unknown dtype");
    if (s.dtype != MRA_F32 && out_dtype != MRA_F32 && s.dtype != out_dtype)
      return fail(MRA_EINVAL, sk + ": f16 <-> bf16 is refused (equal 16-bit types, or f32 on one side)");
    if (s.rows < 0) return fail(MRA_EINVAL, sk + ": negative rows");
    if (s.ld < width) return fail(MRA_EINVAL, sk + ": ld < width");
    if (s.ld % (s.dtype == MRA_F32 ? 4 : 8)) return fail(MRA_EINVAL, sk + ": the pitch must be a multiple of 16 bytes");
    if (!aligned16(s.ptr)) return fail(MRA_EINVAL, sk + ": ptr must be 16-byte aligned");
    ptrs[k] = s.ptr;
    lds[k] = s.ld;
    rows[k] = s.rows;
    dts[k] = s.dtype;   // MRA_F32 / MRA_F16 / MRA_BF16 = 0 / 1 / 2, the kernel's own codes
  }
  return chk(launch_gather_rows(out, ldo, out_dtype, n_rows, width, ptrs, lds, rows, dts, n_src, plan, as_stream(stream)), "gather_rows");
}

}  // extern "C"
