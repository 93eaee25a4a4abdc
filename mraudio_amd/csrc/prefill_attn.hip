// Causal grouped-query attention of the attached LM's prefill: replaces scaled_dot_product_attention under the [Sq][Skv] bool mask inside the
// reference's self.llm_model.generate(inputs_embeds=..., attention_mask=...) (models/xinstructblip.py:388-391), for the first forward over the
// whole prefix.  For query (b, h, i), with G = Hq / Hkv:
//     attended  = {s : s <= q_offset + i, s < Skv, mask[b][s] != 0}
//     z_s       = scale * q[b,h,i] . k[b, h / G, s]            fp32 (MFMA accumulation), attended s only
//     out       = sum_s softmax(z)_s v[b, h / G, s]            P rounded once to the operand type for the MFMA, fp32 sum, one rounding
//     lse       = log sum_s exp z_s                            no attended key: out = +0, lse = -inf
// A workgroup of 4 waves owns PREFILL_QB = 256 query rows of one (b, query head); wave w owns the 32-row blocks w and w + 4 of them (an early
// and a late one: the causal work is balanced over the waves), Q fragments and the O^T accumulators in registers.  K / V tiles of PREFILL_KT =
// 32 keys are staged ONCE per workgroup into a two-deep LDS ring (global loads to registers while the previous tile is computed, one barrier
// per tile) in attention.hip's layout: [tok][64 d] halves of 128-byte rows, K chunks XOR (tok >> 1) & 7 for the b128 fragment reads, V chunks
// XOR ((tok >> 1) & 1) << 2 for the transposed reads.  Per tile and 32-row block:
//     S^T[tok][q] = K Q^T    D / 16 x v_mfma_f32_32x32x16;  per element select (key byte, s <= q_offset + i);  online softmax in log2 units
//     O^T[d][q]  += V^T P^T  D / 16 x v_mfma_f32_32x32x16, P^T is the rounded S^T accumulator, V^T from ds_read_b64_tr_b16
// The key loop of a workgroup ends at the diagonal of its last row; a 32-row block skips the tiles above its own last row; a tile whose key
// bytes are all zero is neither loaded nor computed (the running maximum and sum are not touched).  Masking is a select on both sides: a V row
// of a key that no row of the workgroup attends is staged as zeros, a masked logit is replaced, never added to.  The heaviest (latest) query
// blocks are launched first.  No atomics, no workspace, one launch: two runs give the same bits.
#include "kernels.h"
#include "mra_common.h"

namespace mra {
namespace {

constexpr float PF_L2E = 1.4426950408889634f;
constexpr float PF_LN2 = 0.6931471805599453f;
constexpr int PF_KT = PREFILL_KT;
constexpr int PF_RB = PREFILL_QB / 128;      // 32-row blocks per wave
constexpr int PF_HALF_B = PF_KT * 128;       // bytes of a [32 tok][64 d] half tile
static_assert(PF_KT == 32 && PREFILL_QB % 128 == 0, "the tile step is written for 32 keys and 4 waves of 32-row blocks");

// The first tile t' >= t below nt with an attended key among its 32: bit j of `bits` = key 32 t' + j is below kend and its byte is set.
// Wave-uniform; nt when there is none.
__device__ __forceinline__ int prefill_next_tile(const unsigned char* mrow, int t, int nt, int kend, int lane, unsigned& bits) {
  for (; t < nt; ++t) {
    const int s = t * PF_KT + lane;
    const bool on = lane < PF_KT && s < kend && (!mrow || mrow[s] != 0);
    bits = (unsigned)__ballot(on);
    if (bits) break;
  }
  return t;
}

// grid (Hq, B, query blocks), 256 threads; blockIdx.z = 0 is the LAST query block
template <typename T, int D>
__global__ __launch_bounds__(256) void prefill_attn_kernel(const PrefillArgs a) {
  typedef typename Vec8<T>::type V8;
  constexpr int NH = D / 64;                  // [32][64] halves per tile
  constexpr int KV_B = NH * PF_HALF_B;        // bytes of a K (or V) tile
  __shared__ __attribute__((aligned(16))) char smem[2 * 2 * KV_B];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = blockIdx.x, b = blockIdx.y;
  const int qb = (int)gridDim.z - 1 - (int)blockIdx.z;
  const int q0 = qb * PREFILL_QB;             // < Sq
  const int qend = min(q0 + PREFILL_QB, a.Sq);
  const int kend = a.q_offset + qend;         // keys below it can be attended by a row of this workgroup; <= Skv
  const int nt = (kend + PF_KT - 1) / PF_KT;
  const int hk = h / a.G;
  const unsigned char* mrow = a.mask ? a.mask + (long long)b * a.mask_sb : nullptr;
  const T* kb_g = (const T*)a.k + (long long)b * a.k_sb + (long long)hk * a.k_sh;
  const T* vb_g = (const T*)a.v + (long long)b * a.v_sb + (long long)hk * a.v_sh;

  // ---- Q fragments of the wave's row blocks: lane = row, elements 16 s + 8 (lane >> 5) .. + 7 ----
  V8 qf[PF_RB][D / 16];
  int rowbase[PF_RB];
#pragma unroll
  for (int r = 0; r < PF_RB; ++r) {
    rowbase[r] = q0 + 32 * (wave + 4 * r);
    const int qr = min(rowbase[r] + (lane & 31), a.Sq - 1);     // rows past Sq repeat the last one and are not stored
    const T* qp = (const T*)a.q + (long long)b * a.q_sb + (long long)h * a.q_sh + (long long)qr * a.q_ss + 8 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < D / 16; ++s) qf[r][s] = *reinterpret_cast<const V8*>(qp + 16 * s);
  }

  // ---- staging: thread = (row tid >> 3, physical chunk tid & 7) of every half ----
  const int srow = tid >> 3, sc = tid & 7;
  const int kc = sc ^ ((srow >> 1) & 7);
  const int vc = sc ^ (((srow >> 1) & 1) << 2);
  const int sdst = srow * 128 + sc * 16;
  V8 kreg[NH], vreg[NH];
  auto fetch = [&](int t, unsigned bits) {
    const int tok = min(t * PF_KT + srow, a.Skv - 1);
    const bool keep = (bits >> srow) & 1u;
    const T* kp = kb_g + (long long)tok * a.k_ss;
    const T* vp = vb_g + (long long)tok * a.v_ss;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {
      kreg[hf] = *reinterpret_cast<const V8*>(kp + 64 * hf + 8 * kc);
      V8 x = *reinterpret_cast<const V8*>(vp + 64 * hf + 8 * vc);
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = keep ? x[e] : (T)0.f;   // a key no row attends: its V bits reach nothing
      vreg[hf] = x;
    }
  };
  auto park = [&](int buf) {
    char* st = smem + buf * 2 * KV_B + sdst;
#pragma unroll
    for (int hf = 0; hf < NH; ++hf) {
      *reinterpret_cast<V8*>(st + hf * PF_HALF_B) = kreg[hf];
      *reinterpret_cast<V8*>(st + KV_B + hf * PF_HALF_B) = vreg[hf];
    }
  };

  // ---- fragment read offsets (as attn_kernel) ----
  int koff[4];
  {
    const int r = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) koff[s] = r * 128 + (((2 * s + hh) ^ ((r >> 1) & 7)) << 4);
  }
  int vlane[2];
  {
    const int g = lane >> 4, i = lane & 15, q4 = i >> 2, p = i & 3, hh = lane >> 5;
    const int vrow = 4 * hh + q4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int c = 4 * mt + 2 * (g & 1) + (p >> 1);
      const int pc = c ^ (((q4 >> 1) & 1) << 2);
      vlane[mt] = vrow * 128 + pc * 16 + (p & 1) * 8;
    }
  }

  const float sl2 = a.scale * PF_L2E;
  const int h4 = 4 * (lane >> 5);
  float m_run[PF_RB], l_run[PF_RB];
  f32x16 ot[PF_RB][D / 32];
  int lastkey[PF_RB];                         // the last key slot a row of the block can attend; -1: the block has no row
#pragma unroll
  for (int r = 0; r < PF_RB; ++r) {
    m_run[r] = -1e30f;
    l_run[r] = 0.f;
    lastkey[r] = rowbase[r] < a.Sq ? a.q_offset + min(rowbase[r] + 31, a.Sq - 1) : -1;
#pragma unroll
    for (int m = 0; m < D / 32; ++m)
#pragma unroll
      for (int i = 0; i < 16; ++i) ot[r][m][i] = 0.f;
  }

  unsigned bits = 0, bits_n = 0;
  int t = prefill_next_tile(mrow, 0, nt, kend, lane, bits);
  if (t < nt) fetch(t, bits);
  int buf = 0;
  while (t < nt) {                            // workgroup-uniform: every wave sees the same key bytes
    park(buf);
    __syncthreads();                          // the tile is whole; every wave is done with the tile before the last (the other buffer's next write)
    const int tn = prefill_next_tile(mrow, t + 1, nt, kend, lane, bits_n);
    if (tn < nt) fetch(tn, bits_n);
    const char* kb = smem + buf * 2 * KV_B;
    const char* vb = kb + KV_B;
    const int tok0 = t * PF_KT;
    const unsigned lb = bits >> h4;
#pragma unroll
    for (int r = 0; r < PF_RB; ++r) {
      if (tok0 > lastkey[r]) continue;        // wave-uniform: the tile is wholly above the block's diagonal (or the block is empty)
      // S^T = K Q^T
      f32x16 st;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
      for (int hf = 0; hf < NH; ++hf)
#pragma unroll
        for (int s = 0; s < 4; ++s) st = mfma32<T>(lds_read8<T>(kb + hf * PF_HALF_B + koff[s]), qf[r][4 * hf + s], st);
      // scores in log2 units; element i = 4 g4 + e is key tok0 + 8 g4 + h4 + e under query q_offset + rowbase + (lane & 31)
      const int lim = a.q_offset + rowbase[r] + (lane & 31) - tok0 - h4;
      float mx = -INFINITY;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g4 + e;
          const bool on = ((lb >> (8 * g4 + e)) & 1u) && 8 * g4 + e <= lim;
          const float y = on ? st[i] * sl2 : -INFINITY;
          st[i] = y;
          mx = fmaxf(mx, y);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run[r], mx);                  // finite: the running maximum starts at -1e30
      const float alpha = __builtin_amdgcn_exp2f(m_run[r] - m_new);
      m_run[r] = m_new;
      float psum = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = __builtin_amdgcn_exp2f(st[i] - m_new);  // exp2(-inf) = 0 for a masked element
        st[i] = p;
        psum += p;
      }
      l_run[r] = l_run[r] * alpha + psum;
#pragma unroll
      for (int m = 0; m < D / 32; ++m)
#pragma unroll
        for (int i = 0; i < 16; ++i) ot[r][m][i] *= alpha;
      // P^T fragments (B operand): k-step s uses accumulator registers 8 s .. 8 s + 7
      V8 pf[2];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[s][j] = from_f32<T>(st[8 * s + j]);
      // O^T += V^T P^T
      auto cat = [](i16x4 lo, i16x4 hi) {
        i16x8 v8;
        v8[0] = lo[0]; v8[1] = lo[1]; v8[2] = lo[2]; v8[3] = lo[3];
        v8[4] = hi[0]; v8[5] = hi[1]; v8[6] = hi[2]; v8[7] = hi[3];
        return __builtin_bit_cast(V8, v8);
      };
#pragma unroll
      for (int hf = 0; hf < NH; ++hf)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const char* va = vb + hf * PF_HALF_B + vlane[mt];
          const i16x4 r0 = lds_read_tr4(va), r1 = lds_read_tr4(va + 1024), r2 = lds_read_tr4(va + 2048), r3 = lds_read_tr4(va + 3072);
          ot[r][2 * hf + mt] = mfma32<T>(cat(r0, r1), pf[0], ot[r][2 * hf + mt]);
          ot[r][2 * hf + mt] = mfma32<T>(cat(r2, r3), pf[1], ot[r][2 * hf + mt]);
        }
    }
    t = tn;
    bits = bits_n;
    buf ^= 1;
  }

  // ---- out[b][q][h][d]: lane = query, O^T register i of accumulator m is d = 32 m + 8 (i >> 2) + h4 + (i & 3) ----
#pragma unroll
  for (int r = 0; r < PF_RB; ++r) {
    const int q = rowbase[r] + (lane & 31);
    const float l = l_run[r] + __shfl_xor(l_run[r], 32, 64);
    if (q >= a.Sq) continue;
    const bool any = l > 0.f;                 // an attended key leaves p = 1 at the maximum: l >= 1
    const float inv = any ? 1.0f / l : 0.f;
    T* op = (T*)a.out + (long long)b * a.o_sb + (long long)q * a.o_ss + (long long)h * a.o_sh + h4;
#pragma unroll
    for (int m = 0; m < D / 32; ++m)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        typename Vec4<T>::type x;
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = from_f32<T>(any ? ot[r][m][4 * g4 + e] * inv : 0.f);
        *reinterpret_cast<typename Vec4<T>::type*>(op + 32 * m + 8 * g4) = x;
      }
    if (a.lse && lane < 32) a.lse[((long long)b * a.Hq + h) * a.Sq + q] = any ? m_run[r] * PF_LN2 + logf(l) : -INFINITY;
  }
}

template <typename T, int D>
int launch_t(const PrefillArgs& a, hipStream_t stream) {
  const int nqb = prefill_qblocks(a.Sq);
  hipLaunchKernelGGL((prefill_attn_kernel<T, D>), dim3(a.Hq, a.B, nqb), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace

int launch_prefill_attention(const PrefillArgs& a, int D, int op_dtype, hipStream_t stream) {
  if (a.B <= 0) return 0;
  if (a.Sq < 1 || a.Skv < 1 || a.q_offset < 0 || (long long)a.q_offset + a.Sq > a.Skv || a.Skv > PREFILL_MAX_SKV || a.G < 1 || a.Hq % a.G ||
      (D != 64 && D != 128) || a.B > 65535 || prefill_qblocks(a.Sq) > 65535)
    return -1;
  if (op_dtype == OP_BF16) return D == 64 ? launch_t<bf16, 64>(a, stream) : launch_t<bf16, 128>(a, stream);
  return D == 64 ? launch_t<f16, 64>(a, stream) : launch_t<f16, 128>(a, stream);
}

}  // namespace mra
