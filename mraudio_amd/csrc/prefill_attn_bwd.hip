// Backward of the causal grouped-query attention of prefill_attn.hip: replaces the backward of scaled_dot_product_attention under the
// [S][S] bool mask inside the reference's self.llm_model(inputs_embeds=..., labels=...) (models/xinstructblip.py:599-604), in every layer of
// the attached LM.  With the forward's attended set att(b, i) = {s : s <= q_offset + i, s < Skv, mask[b][s] != 0}, G = Hq / Hkv, the lse of
// the forward (or of any caller) and the cotangent dO:
//     z_is    = scale q[b,h,i] . k[b, h / G, s]                 fp32 (MFMA accumulation)
//     p_is    = exp(z_is - lse_i)                               0 outside att(b, i); a row with lse = -inf has p = 0 everywhere
//     delta_i = sum_d dO[b,i,h,d] out[b,i,h,d]                  fp32
//     dV[b,g,s] = sum_{h in g} sum_i p_is dO[b,i,h]             p rounded once to the operand type for the MFMA
//     ds_is   = p_is (dO[b,i,h] . v[b, h / G, s] - delta_i)     rounded once to the operand type for the MFMAs
//     dQ[b,h,i] = scale sum_s ds_is k[b, h / G, s]      dK[b,g,s] = scale sum_{h in g} sum_i ds_is q[b,h,i]
// Two launches, each the forward's tile machinery (v_mfma_f32_32x32x16, an accumulator as the next product's B operand, the other operand
// through the transposed LDS read) with the roles exchanged.
//   dQ      A workgroup of 4 waves owns PREFILL_BWD_QB = 128 query rows of one (b, query head), a wave one 32-row block with its Q and dO
//           fragments, lse, delta and the dQ^T accumulators in registers.  K / V tiles of 32 keys are staged once per workgroup into a
//           two-deep LDS ring, K twice (the forward's K layout for S^T = K Q^T, its V layout for the transposed read), V in the K layout for
//           dP^T = V dO^T.  dS^T is formed in the accumulator layout, dQ^T += K^T dS^T.  Tiles whose key bytes are all zero are skipped as
//           in the forward.  delta of the rows goes to the workspace.  The heaviest (latest) query blocks are launched first.
//   dK/dV   A workgroup of 4 waves owns PREFILL_BWD_KB = 128 keys of one (b, K/V head), a wave 32 of them with its K and V fragments and
//           the dK^T / dV^T accumulators in registers.  It walks the group's query heads in ascending order, each over the 32-row query
//           tiles from the block's diagonal up to Sq; a tile's Q and dO (each in both LDS layouts), lse and delta are staged once for the
//           four waves.  S = Q K^T, dV^T += dO^T P, dP = dO V^T, dK^T += Q^T dS.  The group sum stays in the accumulators: one rounding.
//           A key block with no attended key writes zeros.  The heaviest (earliest) key blocks are launched first.
// Masking is a select on both sides: a K / V row that no row attends, and the Q / dO / out of a row that attends nothing (lse = -inf), are
// replaced by zeros where they are staged, and p and ds are selected, never multiplied, to zero.  No atomics: two runs give the same bits.
#include "kernels.h"
#include "mra_common.h"

namespace mra {
namespace {

constexpr float PB_L2E = 1.4426950408889634f;
constexpr int PB_KT = 32;
constexpr int PB_HALF_B = PB_KT * 128;       // bytes of a [32 rows][64 d] half tile
static_assert(PREFILL_BWD_QB == 128 && PREFILL_BWD_KB == 128 && PREFILL_BWD_QT == 32, "the kernels are written for 4 waves of 32 rows / keys");

// as prefill_next_tile of prefill_attn.hip
__device__ __forceinline__ int bwd_next_tile(const unsigned char* mrow, int t, int nt, int kend, int lane, unsigned& bits) {
  for (; t < nt; ++t) {
    const int s = t * PB_KT + lane;
    const bool on = lane < PB_KT && s < kend && (!mrow || mrow[s] != 0);
    bits = (unsigned)__ballot(on);
    if (bits) break;
  }
  return t;
}

// the lane parts of the fragment reads: koff, the b128 row-major reads of a tile in the K layout (chunks XOR (row >> 1) & 7); vlane, the
// transposed reads of a tile in the V layout (chunks XOR ((row >> 1) & 1) << 2).  As prefill_attn_kernel.
struct FragOffsets {
  int koff[4], vlane[2];
  __device__ __forceinline__ explicit FragOffsets(int lane) {
    const int r = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) koff[s] = r * 128 + (((2 * s + hh) ^ ((r >> 1) & 7)) << 4);
    const int g = lane >> 4, i = lane & 15, q4 = i >> 2, p = i & 3;
    const int vrow = 4 * hh + q4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int c = 4 * mt + 2 * (g & 1) + (p >> 1);
      const int pc = c ^ (((q4 >> 1) & 1) << 2);
      vlane[mt] = vrow * 128 + pc * 16 + (p & 1) * 8;
    }
  }
};

template <typename T>
__device__ __forceinline__ typename Vec8<T>::type cat_tr(i16x4 lo, i16x4 hi) {
  i16x8 v8;
  v8[0] = lo[0]; v8[1] = lo[1]; v8[2] = lo[2]; v8[3] = lo[3];
  v8[4] = hi[0]; v8[5] = hi[1]; v8[6] = hi[2]; v8[7] = hi[3];
  return __builtin_bit_cast(typename Vec8<T>::type, v8);
}

// acc[m][.] += X^T F over the 32 rows of the tile `xt` (V layout, NH halves): X^T through the transposed read, F the two B fragments
template <typename T, int NH>
__device__ __forceinline__ void mfma_tr(const char* xt, const int (&vlane)[2], const typename Vec8<T>::type (&f)[2], f32x16 (&acc)[2 * NH]) {
#pragma unroll
  for (int hf = 0; hf < NH; ++hf)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const char* va = xt + hf * PB_HALF_B + vlane[mt];
      const i16x4 r0 = lds_read_tr4(va), r1 = lds_read_tr4(va + 1024), r2 = lds_read_tr4(va + 2048), r3 = lds_read_tr4(va + 3072);
      acc[2 * hf + mt] = mfma32<T>(cat_tr<T>(r0, r1), f[0], acc[2 * hf + mt]);
      acc[2 * hf + mt] = mfma32<T>(cat_tr<T>(r2, r3), f[1], acc[2 * hf + mt]);
    }
}

// ---- dQ and delta: grid (Hq, B, query blocks), 256 threads; blockIdx.z = 0 is the LAST query block ----
template <typename T, int D>
__global__ __launch_bounds__(256) void prefill_dq_kernel(const PrefillBwdArgs a) {
  typedef typename Vec8<T>::type V8;
  constexpr int NH = D / 64;
  constexpr int KV_B = NH * PB_HALF_B;
  __shared__ __attribute__((aligned(16))) char smem[2 * 3 * KV_B];   // ring of [K, K layout | K, V layout | V, K layout]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.x, b = blockIdx.y;
  const int qb = (int)gridDim.z - 1 - (int)blockIdx.z;
  const int q0 = qb * PREFILL_BWD_QB;
  const int qend = min(q0 + PREFILL_BWD_QB, a.Sq);
  const int kend = a.q_offset + qend;
  const int nt = (kend + PB_KT - 1) / PB_KT;
  const int hk = h / a.G;
  const unsigned char* mrow = a.mask ? a.mask + (long long)b * a.mask_sb : nullptr;
  const T* kb_g = (const T*)a.k + (long long)b * a.k_sb + (long long)hk * a.k_sh;
  const T* vb_g = (const T*)a.v + (long long)b * a.v_sb + (long long)hk * a.v_sh;
  const int h4 = 4 * (lane >> 5);

  // ---- the wave's 32 rows: Q and dO fragments (lane = row, elements 16 s + 8 (lane >> 5) .. + 7), lse, delta ----
  const int rowbase = q0 + 32 * wave;
  const int q = rowbase + (lane & 31);
  const int qr = min(q, a.Sq - 1);
  const float lse_r = a.lse[((long long)b * a.Hq + h) * a.Sq + qr];
  const bool live = q < a.Sq && lse_r > -INFINITY;            // the row attends a key; its dO and out are read, but reach nothing otherwise
  const float lse2 = lse_r * PB_L2E;
  V8 qf[D / 16], dof[D / 16];
  float delta = 0.f;
  {
    const T* qp = (const T*)a.q + (long long)b * a.q_sb + (long long)h * a.q_sh + (long long)qr * a.q_ss + 8 * (lane >> 5);
    const T* dp = (const T*)a.dout + (long long)b * a.do_sb + (long long)qr * a.do_ss + (long long)h * a.do_sh + 8 * (lane >> 5);
    const T* op = (const T*)a.out + (long long)b * a.o_sb + (long long)qr * a.o_ss + (long long)h * a.o_sh + 8 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      qf[s] = *reinterpret_cast<const V8*>(qp + 16 * s);
      V8 x = *reinterpret_cast<const V8*>(dp + 16 * s);
      const V8 o = *reinterpret_cast<const V8*>(op + 16 * s);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        x[e] = live ? x[e] : (T)0.f;
        delta += live ? (float)x[e] * (float)o[e] : 0.f;
      }
      dof[s] = x;
    }
    delta += __shfl_xor(delta, 32, 64);
    if (lane < 32 && q < a.Sq) a.delta[((long long)b * a.Hq + h) * a.Sq + q] = delta;
  }

  // ---- staging: thread = (key tid >> 3, chunk tid & 7) of every half ----
  const int srow = tid >> 3, sc = tid & 7;
  const int dst_k = srow * 128 + ((sc ^ ((srow >> 1) & 7)) << 4);
  const int dst_v = srow * 128 + ((sc ^ (((srow >> 1) & 1) << 2)) << 4);
  V8 kreg[NH], vreg[NH];
  auto fetch = [&](int t, unsigned bits) {
    const int tok = min(t * PB_KT + srow, a.Skv - 1);
    const bool keep = (bits >> srow) & 1u;
    const T* kp = kb_g + (long long)tok * a.k_ss + 8 * sc;
    const T* vp = vb_g + (long long)tok * a.v_ss + 8 * sc;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {
      V8 x = *reinterpret_cast<const V8*>(kp + 64 * hf);
      V8 y = *reinterpret_cast<const V8*>(vp + 64 * hf);
#pragma unroll
      for (int e = 0; e < 8; ++e) {                            // a key no row of the workgroup attends: its bits reach nothing
        x[e] = keep ? x[e] : (T)0.f;
        y[e] = keep ? y[e] : (T)0.f;
      }
      kreg[hf] = x;
      vreg[hf] = y;
    }
  };
  auto park = [&](int buf) {
    char* st = smem + buf * 3 * KV_B;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {
      *reinterpret_cast<V8*>(st + hf * PB_HALF_B + dst_k) = kreg[hf];
      *reinterpret_cast<V8*>(st + KV_B + hf * PB_HALF_B + dst_v) = kreg[hf];
      *reinterpret_cast<V8*>(st + 2 * KV_B + hf * PB_HALF_B + dst_k) = vreg[hf];
    }
  };

  const FragOffsets fo(lane);
  const float sl2 = a.scale * PB_L2E;
  const int lastkey = rowbase < a.Sq ? a.q_offset + min(rowbase + 31, a.Sq - 1) : -1;
  f32x16 dqt[2 * NH];
#pragma unroll
  for (int m = 0; m < 2 * NH; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) dqt[m][i] = 0.f;

  unsigned bits = 0, bits_n = 0;
  int t = bwd_next_tile(mrow, 0, nt, kend, lane, bits);
  if (t < nt) fetch(t, bits);
  int buf = 0;
  while (t < nt) {                            // workgroup-uniform
    park(buf);
    __syncthreads();
    const int tn = bwd_next_tile(mrow, t + 1, nt, kend, lane, bits_n);
    if (tn < nt) fetch(tn, bits_n);
    const char* kb = smem + buf * 3 * KV_B;
    const char* ktb = kb + KV_B;
    const char* vb = kb + 2 * KV_B;
    const int tok0 = t * PB_KT;
    if (tok0 <= lastkey) {                    // wave-uniform
      f32x16 st, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) { st[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
      for (int hf = 0; hf < NH; ++hf)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          st = mfma32<T>(lds_read8<T>(kb + hf * PB_HALF_B + fo.koff[s]), qf[4 * hf + s], st);      // S^T = K Q^T
          dp = mfma32<T>(lds_read8<T>(vb + hf * PB_HALF_B + fo.koff[s]), dof[4 * hf + s], dp);     // dP^T = V dO^T
        }
      // element i = 4 g4 + e is key tok0 + 8 g4 + h4 + e under query q_offset + q
      const unsigned lb = bits >> h4;
      const int lim = a.q_offset + q - tok0 - h4;
      V8 dsf[2];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g4 + e;
          const bool on = live && ((lb >> (8 * g4 + e)) & 1u) && 8 * g4 + e <= lim;
          const float p = __builtin_amdgcn_exp2f(st[i] * sl2 - lse2);
          dsf[i >> 3][i & 7] = from_f32<T>(on ? p * (dp[i] - delta) : 0.f);
        }
      mfma_tr<T, NH>(ktb, fo.vlane, dsf, dqt);                  // dQ^T += K^T dS^T
    }
    t = tn;
    bits = bits_n;
    buf ^= 1;
  }

  // ---- dq[b][h][q][d]: lane = query, register i of accumulator m is d = 32 m + 8 (i >> 2) + h4 + (i & 3) ----
  if (q < a.Sq) {
    T* op = (T*)a.dq + (long long)b * a.dq_sb + (long long)h * a.dq_sh + (long long)q * a.dq_ss + h4;
#pragma unroll
    for (int m = 0; m < 2 * NH; ++m)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        typename Vec4<T>::type x;
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = from_f32<T>(live ? dqt[m][4 * g4 + e] * a.scale : 0.f);
        *reinterpret_cast<typename Vec4<T>::type*>(op + 32 * m + 8 * g4) = x;
      }
  }
}

// ---- dK and dV: grid (Hkv, B, key blocks), 256 threads; blockIdx.z = 0 is the FIRST key block ----
template <typename T, int D>
__global__ __launch_bounds__(256) void prefill_dkv_kernel(const PrefillBwdArgs a) {
  typedef typename Vec8<T>::type V8;
  constexpr int NH = D / 64;
  constexpr int KV_B = NH * PB_HALF_B;
  __shared__ __attribute__((aligned(16))) char smem[4 * KV_B];       // [Q, K layout | Q, V layout | dO, K layout | dO, V layout]
  __shared__ __attribute__((aligned(16))) float stat[2][PREFILL_BWD_QT];   // lse in log2 units (-inf: the row attends nothing), delta
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.x, b = blockIdx.y;
  const int k0 = (int)blockIdx.z * PREFILL_BWD_KB;                   // < Skv
  const int klast = min(a.Skv, a.q_offset + a.Sq);                   // keys at or behind it are attended by no row
  const unsigned char* mrow = a.mask ? a.mask + (long long)b * a.mask_sb : nullptr;
  const int h4 = 4 * (lane >> 5);

  // ---- the wave's 32 keys: K and V fragments (lane = key, elements 16 s + 8 (lane >> 5) .. + 7); a key no row attends is zeros ----
  const int kbase = k0 + 32 * wave;
  const int key = kbase + (lane & 31);
  const bool klive = key < klast && (!mrow || mrow[key] != 0);
  const bool wlive = __ballot(klive) != 0;                           // wave-uniform
  bool blive = false;                                                // workgroup-uniform: every wave looks at the block's 128 keys
#pragma unroll
  for (int j = 0; j < PREFILL_BWD_KB / 64; ++j) {
    const int s = k0 + 64 * j + lane;
    blive = blive || __ballot(s < klast && (!mrow || mrow[s] != 0)) != 0;
  }
  V8 kf[D / 16], vf[D / 16];
  {
    const int kr = min(key, a.Skv - 1);
    const T* kp = (const T*)a.k + (long long)b * a.k_sb + (long long)g * a.k_sh + (long long)kr * a.k_ss + 8 * (lane >> 5);
    const T* vp = (const T*)a.v + (long long)b * a.v_sb + (long long)g * a.v_sh + (long long)kr * a.v_ss + 8 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < D / 16; ++s) {
      V8 x = *reinterpret_cast<const V8*>(kp + 16 * s);
      V8 y = *reinterpret_cast<const V8*>(vp + 16 * s);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        x[e] = klive ? x[e] : (T)0.f;
        y[e] = klive ? y[e] : (T)0.f;
      }
      kf[s] = x;
      vf[s] = y;
    }
  }

  // ---- the walk: query heads g G .. g G + G - 1 in ascending order, each over the query tiles jt0 .. ntq - 1 ----
  const int ntq = (a.Sq + PREFILL_BWD_QT - 1) / PREFILL_BWD_QT;
  const int jt0 = max(0, k0 - a.q_offset) / PREFILL_BWD_QT;          // the tile of the first row at or past the block's diagonal
  const int ntile = max(0, ntq - jt0);
  const int total = blive ? a.G * ntile : 0;

  // ---- staging: thread = (row tid >> 3, chunk tid & 7) of every half of Q and dO ----
  const int srow = tid >> 3, sc = tid & 7;
  const int dst_k = srow * 128 + ((sc ^ ((srow >> 1) & 7)) << 4);
  const int dst_v = srow * 128 + ((sc ^ (((srow >> 1) & 1) << 2)) << 4);
  V8 qreg[NH], dreg[NH];
  float lse2_reg = -INFINITY, delta_reg = 0.f;
  auto fetch = [&](int idx) {
    const int h = g * a.G + idx / ntile;
    const int qrow = (jt0 + idx % ntile) * PREFILL_BWD_QT + srow;
    const int qr = min(qrow, a.Sq - 1);
    const long long ri = ((long long)b * a.Hq + h) * a.Sq + qr;
    const float l = a.lse[ri];
    const bool live = qrow < a.Sq && l > -INFINITY;
    lse2_reg = live ? l * PB_L2E : -INFINITY;
    delta_reg = live ? a.delta[ri] : 0.f;
    const T* qp = (const T*)a.q + (long long)b * a.q_sb + (long long)h * a.q_sh + (long long)qr * a.q_ss + 8 * sc;
    const T* dp = (const T*)a.dout + (long long)b * a.do_sb + (long long)qr * a.do_ss + (long long)h * a.do_sh + 8 * sc;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {
      V8 x = *reinterpret_cast<const V8*>(qp + 64 * hf);
      V8 y = *reinterpret_cast<const V8*>(dp + 64 * hf);
#pragma unroll
      for (int e = 0; e < 8; ++e) {                            // a row that attends nothing (or past Sq): its bits reach nothing
        x[e] = live ? x[e] : (T)0.f;
        y[e] = live ? y[e] : (T)0.f;
      }
      qreg[hf] = x;
      dreg[hf] = y;
    }
  };
  auto park = [&]() {
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {
      *reinterpret_cast<V8*>(smem + hf * PB_HALF_B + dst_k) = qreg[hf];
      *reinterpret_cast<V8*>(smem + KV_B + hf * PB_HALF_B + dst_v) = qreg[hf];
      *reinterpret_cast<V8*>(smem + 2 * KV_B + hf * PB_HALF_B + dst_k) = dreg[hf];
      *reinterpret_cast<V8*>(smem + 3 * KV_B + hf * PB_HALF_B + dst_v) = dreg[hf];
    }
    if (sc == 0) {
      stat[0][srow] = lse2_reg;
      stat[1][srow] = delta_reg;
    }
  };

  const FragOffsets fo(lane);
  const float sl2 = a.scale * PB_L2E;
  f32x16 dkt[2 * NH], dvt[2 * NH];
#pragma unroll
  for (int m = 0; m < 2 * NH; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dkt[m][i] = 0.f; dvt[m][i] = 0.f; }

  if (total > 0) fetch(0);
  for (int idx = 0; idx < total; ++idx) {     // workgroup-uniform
    __syncthreads();                          // every wave is done with the tile before
    park();
    __syncthreads();                          // the tile is whole
    if (idx + 1 < total) fetch(idx + 1);
    const int qt0 = (jt0 + idx % ntile) * PREFILL_BWD_QT;
    // the wave has an attended key, and the tile's last row sits at or past the wave's first key
    if (!wlive || a.q_offset + min(qt0 + PREFILL_BWD_QT - 1, a.Sq - 1) < kbase) continue;      // wave-uniform
    f32x16 st, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) { st[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
    for (int hf = 0; hf < NH; ++hf)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        st = mfma32<T>(lds_read8<T>(smem + hf * PB_HALF_B + fo.koff[s]), kf[4 * hf + s], st);                // S = Q K^T
        dp = mfma32<T>(lds_read8<T>(smem + 2 * KV_B + hf * PB_HALF_B + fo.koff[s]), vf[4 * hf + s], dp);     // dP = dO V^T
      }
    // element i = 4 g4 + e is query row qt0 + 8 g4 + h4 + e over key `key`: attended when key <= q_offset + row
    const int lim = key - a.q_offset - qt0 - h4;
    V8 pf[2], dsf[2];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const float4 l4 = *reinterpret_cast<const float4*>(&stat[0][8 * g4 + h4]);
      const float4 d4 = *reinterpret_cast<const float4*>(&stat[1][8 * g4 + h4]);
      const float ls[4] = {l4.x, l4.y, l4.z, l4.w}, de[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * g4 + e;
        const bool on = klive && 8 * g4 + e >= lim && ls[e] > -INFINITY;
        const float p = on ? __builtin_amdgcn_exp2f(st[i] * sl2 - ls[e]) : 0.f;
        pf[i >> 3][i & 7] = from_f32<T>(p);
        dsf[i >> 3][i & 7] = from_f32<T>(on ? p * (dp[i] - de[e]) : 0.f);
      }
    }
    mfma_tr<T, NH>(smem + 3 * KV_B, fo.vlane, pf, dvt);         // dV^T += dO^T P
    mfma_tr<T, NH>(smem + KV_B, fo.vlane, dsf, dkt);            // dK^T += Q^T dS
  }

  // ---- dk, dv [b][g][key][d]: lane = key, register i of accumulator m is d = 32 m + 8 (i >> 2) + h4 + (i & 3) ----
  if (key < a.Skv) {
    T* kp = (T*)a.dk + (long long)b * a.dk_sb + (long long)g * a.dk_sh + (long long)key * a.dk_ss + h4;
    T* vp = (T*)a.dv + (long long)b * a.dv_sb + (long long)g * a.dv_sh + (long long)key * a.dv_ss + h4;
#pragma unroll
    for (int m = 0; m < 2 * NH; ++m)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        typename Vec4<T>::type x, y;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x[e] = from_f32<T>(klive ? dkt[m][4 * g4 + e] * a.scale : 0.f);
          y[e] = from_f32<T>(klive ? dvt[m][4 * g4 + e] : 0.f);
        }
        *reinterpret_cast<typename Vec4<T>::type*>(kp + 32 * m + 8 * g4) = x;
        *reinterpret_cast<typename Vec4<T>::type*>(vp + 32 * m + 8 * g4) = y;
      }
  }
}

template <typename T, int D>
int launch_t(const PrefillBwdArgs& a, hipStream_t stream) {
  const int nqb = (a.Sq + PREFILL_BWD_QB - 1) / PREFILL_BWD_QB, nkb = (a.Skv + PREFILL_BWD_KB - 1) / PREFILL_BWD_KB;
  hipLaunchKernelGGL((prefill_dq_kernel<T, D>), dim3(a.Hq, a.B, nqb), dim3(256), 0, stream, a);
  if (hipGetLastError() != hipSuccess) return -4;
  hipLaunchKernelGGL((prefill_dkv_kernel<T, D>), dim3(a.Hq / a.G, a.B, nkb), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace

int launch_prefill_attention_backward(const PrefillBwdArgs& a, int D, int op_dtype, hipStream_t stream) {
  if (a.B <= 0) return 0;
  if (a.Sq < 1 || a.Skv < 1 || a.q_offset < 0 || (long long)a.q_offset + a.Sq > a.Skv || a.Skv > PREFILL_MAX_SKV || a.G < 1 || a.Hq % a.G ||
      (D != 64 && D != 128) || a.B > 65535 || (a.Sq + PREFILL_BWD_QB - 1) / PREFILL_BWD_QB > 65535 ||
      (a.Skv + PREFILL_BWD_KB - 1) / PREFILL_BWD_KB > 65535 || !a.lse || !a.delta)
    return -1;
  if (op_dtype == OP_BF16) return D == 64 ? launch_t<bf16, 64>(a, stream) : launch_t<bf16, 128>(a, stream);
  return D == 64 ? launch_t<f16, 64>(a, stream) : launch_t<f16, 128>(a, stream);
}

}  // namespace mra
