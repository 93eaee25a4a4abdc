// One-token attention of the attached LM's decode: replaces scaled_dot_product_attention with one query row per head behind the reference's
// self.llm_model.generate(inputs_embeds=..., attention_mask=...) (models/xinstructblip.py:383-391), over a K/V cache that is read in place.
//     z_s     = scale * q[b,h] . k[b, h / G, s]          fp32, for the attended keys s only (mask byte != 0; NULL mask: every s < S)
//     out[b,h] = sum_s softmax(z)_s v[b, h / G, s]        fp32 probabilities (never rounded to 16 bits), fp32 sum, one rounding to the dtype
//     lse[b,h] = log sum_s exp z_s                        no attended key: out = +0, lse = -inf
// Memory bound: a workgroup owns (b, kv head, a chunk of DECODE_CHUNK keys) and serves all G = Hq / Hkv query heads of the kv head from ONE
// read of its K and V rows, which go straight to registers as 16-byte loads (D / 8 lanes per key row).  A masked key is never loaded: masking
// is a select, so whatever bits sit in a masked slot (or past S in a longer cache) cannot reach the result.  The chunk's fp32 partials
// (m, l, acc[D]) go to the workspace and a second small launch merges the chunks in ascending order.  No atomics, no counters: two runs give
// the same bits.
#include "kernels.h"
#include "mra_common.h"

namespace mra {
namespace {

constexpr float DA_L2E = 1.4426950408889634f;
constexpr int DA_C = DECODE_CHUNK;

// grid (chunks, Hkv, B), 256 threads.  Lane l of a wave: key row l / L of the wave's step, elements 8 (l % L) .. + 7 (L = D / 8).
template <typename T, int D, int G>
__global__ __launch_bounds__(256) void decode_attn_chunk_kernel(const T* __restrict__ q, long long q_sb, long long q_sh, const T* __restrict__ k,
                                                                long long k_sb, long long k_sh, long long k_ss, const T* __restrict__ v,
                                                                long long v_sb, long long v_sh, long long v_ss,
                                                                const unsigned char* __restrict__ mask, long long mask_sb, int Hq, int S, float scale,
                                                                int nc, float* __restrict__ pm, float* __restrict__ pl, float* __restrict__ pacc) {
  constexpr int L = D / 8;          // lanes per key row
  constexpr int KPW = 64 / L;       // key rows per wave and step
  constexpr int KPI = 4 * KPW;      // key rows per workgroup and step
  constexpr int STEPS = DA_C / KPI;
  __shared__ float zs[G][DA_C];     // logits, then probabilities relative to the chunk maximum
  __shared__ float red[4][G][D];
  __shared__ float ms[G];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kl = lane / L, dp = lane % L;
  const int c = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int s0 = c * DA_C;          // c < nc = ceil(S / DA_C): s0 < S
  const unsigned char* mrow = mask ? mask + (long long)b * mask_sb : nullptr;
  const T* kb = k + (long long)b * k_sb + (long long)hk * k_sh + dp * 8;
  const T* vb = v + (long long)b * v_sb + (long long)hk * v_sh + dp * 8;

  {
    float qf[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const typename Vec8<T>::type x = *reinterpret_cast<const typename Vec8<T>::type*>(q + (long long)b * q_sb + (long long)(hk * G + g) * q_sh + dp * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[g][e] = (float)x[e];
    }
#pragma unroll 4
    for (int i = 0; i < STEPS; ++i) {
      const int j = i * KPI + wave * KPW + kl;
      const long long s = (long long)s0 + j;
      const bool on = s < S && (!mrow || mrow[s] != 0);      // the same for the L lanes of a key row
      float dot[G];
#pragma unroll
      for (int g = 0; g < G; ++g) dot[g] = 0.f;
      if (on) {
        const typename Vec8<T>::type x = *reinterpret_cast<const typename Vec8<T>::type*>(kb + s * k_ss);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int e = 0; e < 8; ++e) dot[g] = fmaf(qf[g][e], (float)x[e], dot[g]);
      }
#pragma unroll
      for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int o = 1; o < L; o <<= 1) dot[g] += __shfl_xor(dot[g], o, 64);
        if (dp == 0) zs[g][j] = on ? scale * dot[g] : -INFINITY;
      }
    }
  }
  __syncthreads();
  // chunk statistics: wave w takes the heads w, w + 4; a lane owns the keys lane, lane + 64, ...
  for (int g = wave; g < G; g += 4) {
    float z[DA_C / 64];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < DA_C / 64; ++t) {
      z[t] = zs[g][lane + 64 * t];
      m = fmaxf(m, z[t]);
    }
    m = wave_max(m);
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < DA_C / 64; ++t) {
      const float p = z[t] > -INFINITY ? __builtin_amdgcn_exp2f((z[t] - m) * DA_L2E) : 0.f;   // an attended key has m >= z > -inf
      zs[g][lane + 64 * t] = p;
      l += p;
    }
    l = wave_sum(l);
    if (lane == 0) {
      const long long row = ((long long)b * Hq + hk * G + g) * nc + c;
      pm[row] = m;
      pl[row] = l;
    }
  }
  __syncthreads();
  float acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
#pragma unroll 4
  for (int i = 0; i < STEPS; ++i) {
    const int j = i * KPI + wave * KPW + kl;
    const long long s = (long long)s0 + j;
    const bool on = s < S && (!mrow || mrow[s] != 0);
    if (on) {
      const typename Vec8<T>::type x = *reinterpret_cast<const typename Vec8<T>::type*>(vb + s * v_ss);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float p = zs[g][j];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = fmaf(p, (float)x[e], acc[g][e]);
      }
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a = acc[g][e];
#pragma unroll
      for (int o = L; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
      if (kl == 0) red[wave][g][dp * 8 + e] = a;
    }
  __syncthreads();
  for (int idx = tid; idx < G * D; idx += 256) {
    const int g = idx / D, d = idx % D;
    const float a = ((red[0][g][d] + red[1][g][d]) + red[2][g][d]) + red[3][g][d];
    pacc[(((long long)b * Hq + hk * G + g) * nc + c) * D + d] = a;
  }
}

// grid (Hq, B), 64 threads; a thread owns D / 64 output columns and walks the chunks in ascending order.  A chunk without an attended key
// (m = -inf) is skipped by a select: no exp(-inf - (-inf)).
template <typename T, int D>
__global__ __launch_bounds__(64) void decode_attn_merge_kernel(const float* __restrict__ pm, const float* __restrict__ pl,
                                                               const float* __restrict__ pacc, int Hq, int nc, T* __restrict__ out, long long o_sb,
                                                               long long o_sh, float* __restrict__ lse) {
  constexpr int E = D / 64;
  const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const long long row = ((long long)b * Hq + h) * nc;
  float M = -INFINITY;
  for (int c = 0; c < nc; ++c) M = fmaxf(M, pm[row + c]);
  float l = 0.f, a[E];
#pragma unroll
  for (int e = 0; e < E; ++e) a[e] = 0.f;
  for (int c = 0; c < nc; ++c) {
    const float m = pm[row + c];
    if (m > -INFINITY) {
      const float w = __builtin_amdgcn_exp2f((m - M) * DA_L2E);
      l = fmaf(pl[row + c], w, l);
#pragma unroll
      for (int e = 0; e < E; ++e) a[e] = fmaf(pacc[(row + c) * D + lane + 64 * e], w, a[e]);
    }
  }
  const bool any = M > -INFINITY;
  T* o = out + (long long)b * o_sb + (long long)h * o_sh;
#pragma unroll
  for (int e = 0; e < E; ++e) o[lane + 64 * e] = from_f32<T>(any ? a[e] / l : 0.f);
  if (lse && lane == 0) lse[(long long)b * Hq + h] = any ? M + logf(l) : -INFINITY;
}

template <typename T, int D, int G>
void launch_chunks(const DecodeArgs& a, int nc, hipStream_t stream) {
  hipLaunchKernelGGL((decode_attn_chunk_kernel<T, D, G>), dim3(nc, a.Hkv, a.B), dim3(256), 0, stream, (const T*)a.q, a.q_sb, a.q_sh, (const T*)a.k,
                     a.k_sb, a.k_sh, a.k_ss, (const T*)a.v, a.v_sb, a.v_sh, a.v_ss, a.mask, a.mask_sb, a.Hq, a.S, a.scale, nc, a.pm, a.pl, a.pacc);
}

template <typename T, int D>
int launch_typed(const DecodeArgs& a, hipStream_t stream) {
  const int nc = decode_chunks(a.S);
  switch (a.Hq / a.Hkv) {
    case 1: launch_chunks<T, D, 1>(a, nc, stream); break;
    case 2: launch_chunks<T, D, 2>(a, nc, stream); break;
    case 4: launch_chunks<T, D, 4>(a, nc, stream); break;
    case 8: launch_chunks<T, D, 8>(a, nc, stream); break;
    default: return -1;
  }
  hipLaunchKernelGGL((decode_attn_merge_kernel<T, D>), dim3(a.Hq, a.B), dim3(64), 0, stream, a.pm, a.pl, a.pacc, a.Hq, nc, (T*)a.out, a.o_sb, a.o_sh,
                     a.lse);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace

int launch_decode_attention(const DecodeArgs& a, int D, int op_dtype, hipStream_t stream) {
  if (a.B <= 0) return 0;
  if (a.S < 1 || a.Hkv < 1 || a.Hq % a.Hkv || (D != 64 && D != 128) || a.B > 65535 || a.Hkv > 65535) return -1;
  if (op_dtype == OP_BF16) return D == 64 ? launch_typed<bf16, 64>(a, stream) : launch_typed<bf16, 128>(a, stream);
  return D == 64 ? launch_typed<f16, 64>(a, stream) : launch_typed<f16, 128>(a, stream);
}

}  // namespace mra
