// The LM objective's vocabulary head and cross-entropy on the labelled rows only: replaces lm_head + ForCausalLMLoss behind the reference's
// self.llm_model(inputs_embeds=..., attention_mask=..., return_dict=True, labels=targets) (models/xinstructblip.py:599-604).
//     z       = h W^T                            h [R][K] gathered hidden rows, W [V][K] as lm_head.weight is stored, fp32 accumulation, z never rounded
//     lse_r   = log sum_v exp z_rv               split softmax: a workgroup owns a 64-column vocabulary tile and leaves the tile maximum m_rt, the
//     nll_r   = lse_r - z_r,y_r                  tile sum s_rt = sum_v exp(z_rv - m_rt) (fp32, unrounded terms) and P~_rv = op(exp(z_rv - m_rt))
//     dh_r    = g_r (softmax(z_r) - e_y_r) W     = sum_t f_rt (sum_{v in t} P~_rv W_v) - g_r W_y_r with the fp32 row factor f_rt = g_r exp(m_rt - lse_r)
// This is the folded cross-attention with the vocabulary embeddings as the tokens: the backward needs no second logits pass, and W is read as
// stored by both products (k-contiguous fragments forward, the LDS transpose read backward).  No atomics: the contraction over V is split into
// `splits` ranges of whole tiles whose fp32 partial sums go to the workspace and are added in ascending split order.
#include "kernels.h"
#include "mra_common.h"

namespace mra {
namespace {

constexpr float LMH_L2E = 1.4426950408889634f;
constexpr int LMH_TV = LM_HEAD_TILE;     // vocabulary columns per tile
constexpr int LMH_RG = LM_HEAD_ROWS;     // rows per workgroup: 8 MFMA row tiles
constexpr int LMH_KB = LM_HEAD_KBLOCK;   // hidden columns per backward workgroup
constexpr int LMH_WP = LMH_KB * 2 + 16;  // LDS pitch of the backward's W tile, bytes

template <typename T> __device__ __forceinline__ f32x4 mfma_bits(i16x8 a, i16x8 b, f32x4 c) {
  return mfma16<T>(__builtin_bit_cast(typename Vec8<T>::type, a), __builtin_bit_cast(typename Vec8<T>::type, b), c);
}

// grid (tiles, row groups).  Wave w owns the tile's columns 16 w .. 16 w + 15 for every row tile of the group: W is streamed once per row group,
// h (small) comes through the caches.  Both fragments are 8 consecutive k of one row: 16-byte global loads, no LDS before the epilogue.
template <typename T>
__global__ __launch_bounds__(256) void lm_head_fwd_kernel(const T* __restrict__ H, long long ldh, int R, int K, const T* __restrict__ W, long long ldw,
                                                          int V, const int* __restrict__ labels, int nt, float* __restrict__ tmax,
                                                          float* __restrict__ tsum, float* __restrict__ zy, T* __restrict__ P, long long ldp) {
  __shared__ float zs[LMH_RG][LMH_TV + 1];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c16 = lane & 15, g = lane >> 4;
  const int tile = blockIdx.x, v0 = tile * LMH_TV;
  const int r0 = blockIdx.y * LMH_RG;
  const int nrows = min(LMH_RG, R - r0), nrt = (nrows + 15) / 16;
  const int vcol = v0 + 16 * wave + c16;
  const bool col_ok = vcol < V;
  const T* wrow = W + (long long)(col_ok ? vcol : 0) * ldw;
  f32x4 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int k0 = 0; k0 < K; k0 += 32) {
    const int k = k0 + g * 8;
    const bool k_ok = k < K;   // K % 8 == 0: a group of 8 is whole or absent
    i16x8 b = {0, 0, 0, 0, 0, 0, 0, 0};
    if (col_ok && k_ok) b = *reinterpret_cast<const i16x8*>(wrow + k);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i < nrt) {
        const int r = r0 + i * 16 + c16;
        i16x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (r < R && k_ok) a = *reinterpret_cast<const i16x8*>(H + (long long)r * ldh + k);
        acc[i] = mfma_bits<T>(a, b, acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (i < nrt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) zs[i * 16 + 4 * g + e][16 * wave + c16] = acc[i][e];
    }
  __syncthreads();
  // statistics: one wave per row, one lane per column; the ragged tail past V is left out of maximum and sum (not zero-filled)
  const int v = v0 + lane;
  const bool v_ok = v < V;
  for (int rr = wave; rr < nrows; rr += 4) {
    const int r = r0 + rr;
    const float z = zs[rr][lane];
    const float m = wave_max(v_ok ? z : -INFINITY);
    const float e = v_ok ? __builtin_amdgcn_exp2f((z - m) * LMH_L2E) : 0.f;
    const float s = wave_sum(e);
    if (P) P[(long long)r * ldp + v] = from_f32<T>(e);   // ldp = 64 nt: the tail columns are inside the row and hold zero
    if (lane == 0) {
      tmax[(long long)r * nt + tile] = m;
      tsum[(long long)r * nt + tile] = s;
    }
    if (v_ok && labels[r] == v) zy[r] = z;   // exactly one lane of one tile owns the label; a label outside [0, V) is owned by none
  }
}

// one wave per row: M = max_t m_t, S = sum_t s_t exp(m_t - M) with lane l adding tiles l, l + 64, ... in ascending order and the 64 lane sums
// merged by the xor butterfly -- a fixed order.  lse = M + log S, nll = lse - z_y (NaN for a label outside [0, V)).
__global__ __launch_bounds__(256) void lm_head_merge_kernel(const float* __restrict__ tmax, const float* __restrict__ tsum, const float* __restrict__ zy,
                                                            const int* __restrict__ labels, int R, int V, int nt, float* __restrict__ nll,
                                                            float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;   // wave uniform
  const float* mr = tmax + (long long)r * nt;
  const float* sr = tsum + (long long)r * nt;
  float m = -INFINITY;
  for (int t = lane; t < nt; t += 64) m = fmaxf(m, mr[t]);
  m = wave_max(m);
  float s = 0.f;
  for (int t = lane; t < nt; t += 64) s += sr[t] * __builtin_amdgcn_exp2f((mr[t] - m) * LMH_L2E);
  s = wave_sum(s);
  if (lane == 0) {
    const float l = m + logf(s);
    const int y = labels[r];
    lse[r] = l;
    nll[r] = (y >= 0 && y < V) ? l - zy[r] : __builtin_nanf("");
  }
}

// grid (K blocks of 128, splits, row groups).  Per tile of its split the workgroup stages W[64 v][128 k] in LDS as stored; wave w takes the
// hidden columns 32 w .. 32 w + 31 as two B operands through the transposed read (rows = v, the contraction), P~ is the A operand straight from
// the workspace.  The tile's product lands in a temporary and is added with the fp32 row factor: acc += f_rt * tmp.
template <typename T>
__global__ __launch_bounds__(256) void lm_head_bwd_kernel(const float* __restrict__ gr, const T* __restrict__ W, long long ldw, int V, int K,
                                                          const float* __restrict__ lse, const float* __restrict__ tmax, const T* __restrict__ P,
                                                          long long ldp, int R, int nt, int tps, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) char ws[LMH_TV * LMH_WP];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g = lane >> 4;
  const int kb0 = blockIdx.x * LMH_KB;
  const int split = blockIdx.y;
  const int r0 = blockIdx.z * LMH_RG;
  const int nrows = min(LMH_RG, R - r0), nrt = (nrows + 15) / 16;
  const int t_begin = split * tps, t_end = min(nt, t_begin + tps);
  // lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3 of a 4 x 16 block; the group's blocks start at rows 8 g and 8 g + 4
  const int tr_off = (8 * g + (c16 >> 2)) * LMH_WP + (c16 & 3) * 8 + wave * 64;
  f32x4 acc[8][2];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int t = t_begin; t < t_end; ++t) {
    const int v0 = t * LMH_TV;
    __syncthreads();   // the previous tile's reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ch = tid + 256 * i;            // 1024 chunks of 16 bytes: row ch >> 4, chunk ch & 15
      const int row = ch >> 4, kc = (ch & 15) * 8;
      i16x8 w = {0, 0, 0, 0, 0, 0, 0, 0};      // rows past V and columns past K are zero: they meet P~ = 0 and unused outputs
      if (v0 + row < V && kb0 + kc < K) w = *reinterpret_cast<const i16x8*>(W + (long long)(v0 + row) * ldw + kb0 + kc);
      *reinterpret_cast<i16x8*>(ws + row * LMH_WP + kc * 2) = w;
    }
    __syncthreads();
    i16x8 b[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const char* p = ws + tr_off + ks * 32 * LMH_WP + c * 32;
        const i16x4 lo = lds_read_tr4(p), hi = lds_read_tr4(p + 4 * LMH_WP);
        b[ks][c] = i16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i < nrt) {
        const int ra = r0 + i * 16 + c16;
        i16x8 a0 = {0, 0, 0, 0, 0, 0, 0, 0}, a1 = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ra < R) {
          const T* pr = P + (long long)ra * ldp + v0 + g * 8;
          a0 = *reinterpret_cast<const i16x8*>(pr);
          a1 = *reinterpret_cast<const i16x8*>(pr + 32);
        }
        float f[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = r0 + i * 16 + 4 * g + e;
          f[e] = r < R ? gr[r] * __builtin_amdgcn_exp2f((tmax[(long long)r * nt + t] - lse[r]) * LMH_L2E) : 0.f;
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          f32x4 tmp = mfma_bits<T>(a0, b[0][c], f32x4{0.f, 0.f, 0.f, 0.f});
          tmp = mfma_bits<T>(a1, b[1][c], tmp);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][c][e] = fmaf(f[e], tmp[e], acc[i][c][e]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (i < nrt) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int k = kb0 + 32 * wave + 16 * c + c16;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = r0 + i * 16 + 4 * g + e;
          if (r < R && k < K) part[((long long)split * R + r) * K + k] = acc[i][c][e];
        }
      }
    }
}

// dh[r][k] = op(sum_s part[s][r][k] (s ascending) - g_r W[y_r][k]); a thread owns 8 columns.  The one-hot term is subtracted in fp32, before
// the only rounding; a label outside [0, V) has none.
template <typename T>
__global__ __launch_bounds__(256) void lm_head_reduce_kernel(const float* __restrict__ part, int splits, const float* __restrict__ gr,
                                                             const T* __restrict__ W, long long ldw, int V, int K, const int* __restrict__ labels,
                                                             T* __restrict__ dh, long long lddh, int R) {
  const int kc = K >> 3;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)R * kc) return;
  const int r = (int)(idx / kc), k = (int)(idx - (long long)r * kc) * 8;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int sp = 0; sp < splits; ++sp) {
    const float4* p = reinterpret_cast<const float4*>(part + ((long long)sp * R + r) * K + k);
    const float4 x = p[0], y = p[1];
    s[0] += x.x; s[1] += x.y; s[2] += x.z; s[3] += x.w; s[4] += y.x; s[5] += y.y; s[6] += y.z; s[7] += y.w;
  }
  const int y = labels[r];
  if (y >= 0 && y < V) {
    const float gy = gr[r];
    const T* wy = W + (long long)y * ldw + k;
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = fmaf(-gy, (float)wy[e], s[e]);
  }
  i16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = __builtin_bit_cast(short, from_f32<T>(s[e]));
  *reinterpret_cast<i16x8*>(dh + (long long)r * lddh + k) = o;
}

}  // namespace

int launch_lm_head_fwd(const void* H, long long ldh, int R, int K, const void* W, long long ldw, int V, const int* labels, float* nll, float* lse,
                       float* tmax, float* tsum, float* zy, void* P, int op_dtype, hipStream_t stream) {
  if (R <= 0) return 0;
  if (K <= 0 || K % 8 || V < 1 || ldh < K || ldh % 8 || ldw < K || ldw % 8) return -1;
  const int nt = lm_head_tiles(V);
  const long long ldp = (long long)nt * LMH_TV;
  const dim3 grid(nt, (R + LMH_RG - 1) / LMH_RG), block(256);
  if (op_dtype == OP_BF16)
    hipLaunchKernelGGL(lm_head_fwd_kernel<bf16>, grid, block, 0, stream, (const bf16*)H, ldh, R, K, (const bf16*)W, ldw, V, labels, nt, tmax, tsum, zy,
                       (bf16*)P, ldp);
  else
    hipLaunchKernelGGL(lm_head_fwd_kernel<f16>, grid, block, 0, stream, (const f16*)H, ldh, R, K, (const f16*)W, ldw, V, labels, nt, tmax, tsum, zy,
                       (f16*)P, ldp);
  hipLaunchKernelGGL(lm_head_merge_kernel, dim3((R + 3) / 4), block, 0, stream, tmax, tsum, zy, labels, R, V, nt, nll, lse);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_lm_head_bwd(const float* g, const void* W, long long ldw, int V, int K, const int* labels, const float* lse, const float* tmax,
                       const void* P, float* part, void* dh, long long lddh, int R, int op_dtype, hipStream_t stream) {
  if (R <= 0) return 0;
  if (K <= 0 || K % 8 || V < 1 || ldw < K || ldw % 8 || lddh < K || lddh % 8) return -1;
  const int nt = lm_head_tiles(V), splits = lm_head_splits(R, V, K), tps = (nt + splits - 1) / splits;
  const long long ldp = (long long)nt * LMH_TV;
  const dim3 grid((K + LMH_KB - 1) / LMH_KB, splits, (R + LMH_RG - 1) / LMH_RG), block(256);
  const dim3 rgrid((unsigned)(((long long)R * (K / 8) + 255) / 256));
  if (op_dtype == OP_BF16) {
    hipLaunchKernelGGL(lm_head_bwd_kernel<bf16>, grid, block, 0, stream, g, (const bf16*)W, ldw, V, K, lse, tmax, (const bf16*)P, ldp, R, nt, tps, part);
    hipLaunchKernelGGL(lm_head_reduce_kernel<bf16>, rgrid, block, 0, stream, part, splits, g, (const bf16*)W, ldw, V, K, labels, (bf16*)dh, lddh, R);
  } else {
    hipLaunchKernelGGL(lm_head_bwd_kernel<f16>, grid, block, 0, stream, g, (const f16*)W, ldw, V, K, lse, tmax, (const f16*)P, ldp, R, nt, tps, part);
    hipLaunchKernelGGL(lm_head_reduce_kernel<f16>, rgrid, block, 0, stream, part, splits, g, (const f16*)W, ldw, V, K, labels, (f16*)dh, lddh, R);
  }
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace mra
