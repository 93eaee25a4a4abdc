// Row kernels of the folded cross-attention (mra_abi.hip: cross_fold): with Kv >> hidden it is cheaper to
// move W_k / W_v to the query side than to project every encoder token,
//     scores  S = (Q W_k) enc^T        P = softmax(S / 8)        ctx = (P enc) W_v^T + b_v
// (the key bias adds one constant per query row and cancels in the softmax).  The two big products are
// batched GEMMs on the existing tiles (gemm.hip); this file holds what is left:
//   softmax_rows_kernel   fp32 score rows [rows][ld_s] -> P rows [rows][ld_p] in the operand dtype, padding zeroed
//   transpose_pad_kernel  batched [R][C] -> [C][ld_d] transpose with zeroed padding columns: enc -> enc^T per item
//                         (the K-contiguous B operand of P . enc) and W_k -> per-head [E][64] blocks
//   fold_query_kernel     cross query projection + per-head Q' = Q_h W_k,h in one launch (the default folded plan)
// Reference arithmetic: HF modeling_instructblip.py:464-515 (the same softmax(QK^T/8)V, re-associated).
#include <atomic>

#include "kernels.h"
#include "mra_common.h"

namespace mra {

namespace {

constexpr float LOG2E_F = 1.4426950408889634f;

// One workgroup per row.  NV > 0: the row (kv <= 1024 * NV floats) stays in registers, NV float4 per thread --
// one read, one write; NV == 0: any length, three passes over the row (the later ones hit L2).
template <typename T, int NV>
__global__ void __launch_bounds__(256) softmax_rows_kernel(const float* S, long long ld_s, T* P, long long ld_p, int kv, int kvp,
                                                           float sl2) {
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* s = S + (long long)blockIdx.x * ld_s;
  T* p = P + (long long)blockIdx.x * ld_p;
  constexpr int NR = NV > 0 ? NV : 1;
  f32x4 v[NR];
  float m = -3.0e38f;
  if constexpr (NV > 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = 4 * (tid + j * 256);
      if (c + 3 < kv) {
        v[j] = *reinterpret_cast<const f32x4*>(s + c);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[j][e] = c + e < kv ? s[c + e] : -3.0e38f;
      }
      m = fmaxf(fmaxf(m, fmaxf(v[j][0], v[j][1])), fmaxf(v[j][2], v[j][3]));
    }
  } else {
    for (int i = tid; i < kv; i += 256) m = fmaxf(m, s[i]);
  }
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * sl2;
  float l = 0.f;
  if constexpr (NV > 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[j][e] = __builtin_amdgcn_exp2f(v[j][e] * sl2 - m);   // masked tail: exp2(-huge) = 0
        l += v[j][e];
      }
  } else {
    for (int i = tid; i < kv; i += 256) l += __builtin_amdgcn_exp2f(s[i] * sl2 - m);
  }
  l = wave_sum(l);
  if (lane == 0) red[4 + wave] = l;
  __syncthreads();
  const float inv = 1.0f / ((red[4] + red[5]) + (red[6] + red[7]));
  // normalised probabilities; columns [kv, kvp) are zeroed (they meet finite enc^T padding in the next GEMM)
  if constexpr (NV > 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int c = 4 * (tid + j * 256);
      if (c < kvp) {
        typename Vec4<T>::type o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(v[j][e] * inv);
        *reinterpret_cast<typename Vec4<T>::type*>(p + c) = o;
      }
    }
  } else {
    for (int i = tid; i < kvp; i += 256) p[i] = from_f32<T>(i < kv ? __builtin_amdgcn_exp2f(s[i] * sl2 - m) * inv : 0.f);
  }
}

// Second half of the split softmax.  The scores GEMM (EPI_SOFTPART) left P~ = exp2(s - m_tile) per column tile and the
// tile statistics (m_tile, l_tile) of every row; here one workgroup per row finds m_row = max m_tile,
// L = sum exp2(m_tile - m_row) l_tile and rescales the row in place by g_tile = exp2(m_tile - m_row) / L.
// Columns from ntiles * tile_cols to kvp were never written by the GEMM and are zeroed.
// PROBE: also adds the row's softmax maximum 1 / L to the 256-bin histogram hist[256] of [0, 1] (one global atomic per row, i.e. per
// workgroup; see fold_rowfactor_kernel).  P is the plain kernel's, bit for bit.
template <typename T, bool PROBE>
__global__ void __launch_bounds__(256) softmax_rescale_kernel(T* P, long long ld_p, const float* stat_m, const float* stat_l, int ntiles,
                                                              int tile_cols, int kvp, int* hist) {
  __shared__ float g[128];
  const int tid = threadIdx.x;
  const float* sm = stat_m + (long long)blockIdx.x * ntiles;
  const float* sl = stat_l + (long long)blockIdx.x * ntiles;
  if (tid < 64) {
    float m = -3.0e38f;
    for (int t = tid; t < ntiles; t += 64) m = fmaxf(m, sm[t]);
    m = wave_max(m);
    float l = 0.f;
    for (int t = tid; t < ntiles; t += 64) l += __builtin_amdgcn_exp2f(sm[t] - m) * sl[t];
    l = wave_sum(l);
    const float inv = 1.0f / l;
    for (int t = tid; t < ntiles; t += 64) g[t] = __builtin_amdgcn_exp2f(sm[t] - m) * inv;
    if constexpr (PROBE) {
      if (tid == 0) atomicAdd(hist + (int)fminf(fmaxf(inv * 256.f, 0.f), 255.f), 1);   // fmaxf maps a NaN to bin 0
    }
  }
  __syncthreads();
  using V8 = typename Vec8<T>::type;
  T* p = P + (long long)blockIdx.x * ld_p;
  const int cpt = tile_cols >> 3;   // 16-byte chunks per tile
  for (int c = tid; c < (kvp >> 3); c += 256) {
    const int t = c / cpt;
    V8 v;
    if (t < ntiles) {
      v = *reinterpret_cast<const V8*>(p + 8 * c);
      const float s = g[t];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = from_f32<T>((float)v[e] * s);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = from_f32<T>(0.f);
    }
    *reinterpret_cast<V8*>(p + 8 * c) = v;
  }
}

// The same row statistics as softmax_rescale_kernel, but only the factors leave: one wave per row, factors in the [item][tile][512] layout
// the P . enc GEMM's loader waves copy into LDS one tile slice (2 KB) at a time.
// It also zeroes the row's P~ columns from ntiles * tile_cols to kvp, which the scores GEMM never writes and the P . enc GEMM reads
// (its K runs to kvp): zero times any finite factor is zero, so that GEMM needs no column test of its own.
// PROBE (automatic cross-attention precision, mra_qformer_set_cross_precision 2): the row's softmax maximum is exactly 1 / L (the entry at
// s = m_row); each wave bins it into a 256-bin LDS histogram of [0, 1], and the workgroup adds its non-empty bins to hist[256] with one
// global atomic each.  Factors and P are the plain kernel's, bit for bit.
template <bool PROBE>
__global__ void __launch_bounds__(256) fold_rowfactor_kernel(const float* stat_m, const float* stat_l, float* factors, int rows, int R, int ntiles,
                                                             unsigned short* P, long long ld_p, int tile_cols, int kvp, int* hist) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  __shared__ int bins[PROBE ? 256 : 1];
  if constexpr (PROBE) {
    bins[threadIdx.x] = 0;
    __syncthreads();
  }
  if (row < rows) {
    for (int c = ntiles * tile_cols + lane; c < kvp; c += 64) P[(long long)row * ld_p + c] = 0;
    const float* sm = stat_m + (long long)row * ntiles;
    const float* sl = stat_l + (long long)row * ntiles;
    float m = -3.0e38f;
    for (int t = lane; t < ntiles; t += 64) m = fmaxf(m, sm[t]);
    m = wave_max(m);
    float l = 0.f;
    for (int t = lane; t < ntiles; t += 64) l += __builtin_amdgcn_exp2f(sm[t] - m) * sl[t];
    l = wave_sum(l);
    const float inv = 1.0f / l;
    const int item = row / R, r = row - item * R;
    for (int t = lane; t < ntiles; t += 64) factors[((long long)item * ntiles + t) * 512 + r] = __builtin_amdgcn_exp2f(sm[t] - m) * inv;
    if constexpr (PROBE) {
      if (lane == 0) atomicAdd(&bins[(int)fminf(fmaxf(inv * 256.f, 0.f), 255.f)], 1);   // fmaxf maps a NaN to bin 0
    }
  }
  if constexpr (PROBE) {
    __syncthreads();
    const int n = bins[threadIdx.x];
    if (n) atomicAdd(hist + threadIdx.x, n);
  }
}

// dst[b][c][r] = src[b][r][c] for r < R, 0 for R <= r < ld_d; 32 x 32 tiles, grid (ceil(C/32), ceil(ld_d/32), batch)
template <typename T>
__global__ void __launch_bounds__(256) transpose_pad_kernel(const T* src, T* dst, int R, int C, int ld_d, long long src_bs,
                                                            long long dst_bs) {
  __shared__ T tile[32][33];
  src += (long long)blockIdx.z * src_bs;
  dst += (long long)blockIdx.z * dst_bs;
  const int bx = blockIdx.x * 32, by = blockIdx.y * 32;   // bx: source column block, by: source row block
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int j = ty; j < 32; j += 8)
    tile[j][tx] = (by + j < R && bx + tx < C) ? src[(long long)(by + j) * C + bx + tx] : from_f32<T>(0.f);
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (bx + j < C && by + tx < ld_d) dst[(long long)(bx + j) * ld_d + by + tx] = tile[tx][j];
}

// 64 x 64 tiles with 16-byte global accesses (C % 8 == 0, ld_d % 8 == 0): thread t loads chunk (t & 7) of rows
// (t >> 3) and (t >> 3) + 32, then stores chunk (t & 7) of destination rows (t >> 3), (t >> 3) + 32.
template <typename T>
__global__ void __launch_bounds__(256) transpose_pad64_kernel(const T* src, T* dst, int R, int C, int ld_d, long long src_bs,
                                                              long long dst_bs) {
  __shared__ T tile[64][72];   // 144-byte pitch: 16-byte aligned rows
  src += (long long)blockIdx.z * src_bs;
  dst += (long long)blockIdx.z * dst_bs;
  const int bx = blockIdx.x * 64, by = blockIdx.y * 64;   // bx: source column block, by: source row block
  const int ch = (threadIdx.x & 7) * 8, r0 = threadIdx.x >> 3;
  using V8 = typename Vec8<T>::type;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = r0 + 32 * i;
    V8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = from_f32<T>(0.f);
    if (by + r < R && bx + ch < C) v = *reinterpret_cast<const V8*>(src + (long long)(by + r) * C + bx + ch);
    *reinterpret_cast<V8*>(&tile[r][ch]) = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = r0 + 32 * i;       // destination row = source column bx + c
    if (bx + c < C && by + ch < ld_d) {
      V8 v;
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = tile[ch + e][c];
      *reinterpret_cast<V8*>(dst + (long long)(bx + c) * ld_d + by + ch) = v;
    }
  }
}

// Cross query projection and Q' of the folded cross-attention in ONE launch (steps 5 + 6a; mra_qformer_set_option "cross_fuse" bit 1).
// One workgroup per (128-row tile of the compact query rows, head, slice of E); 4 waves.
//   phase 1  Q_h = X W_cq,h^T + b_cq,h for the tile: gemm_kernel's two-buffer loop on a 64 (weight rows of the head) x 128 tile, K = hidden in
//            64-deep steps, fp32 accumulators, + bias, rounded to the operand dtype -- into LDS, laid out as the K = 64 activation tile of
//            phase 2 (128-byte rows, chunk index XOR (row >> 1) & 7).  Q never reaches HBM.
//   phase 2  Q'_h = Q_h W_k,h for the slice's 128-column blocks of E, ONE 64-deep step each.  Up to three blocks of W_k,h [128][64] are brought
//            into LDS at once (LDS-DMA, one wait); then every wave works alone on its 32 rows: Q_h fragments in registers, per 64-column half
//            block 16 MFMAs, its 32 x 64 result through its own 4 KB of LDS and out as whole 16-byte pieces of 128-byte lines into
//            Q' [N][head * 32 + q][E].  No wait on a store and no workgroup barrier inside a group: the stores only queue.  (A first form that
//            exchanged one block per barrier pair and waited for the previous block's stores ran 23.6 us at the headline shape.)
// Both phases issue the MFMAs of the two launches they replace on the same operands in the same ascending K order (an output element is one
// accumulator chain from zero, 32 k per instruction; the bias is one fp32 add), so Q' is theirs bit for bit.  A phase-1 tile is recomputed by
// every slice of E (4 of 3 blocks at E = 1408: 384 workgroups, two of them fit a CU): 294 KB from L2 against the 96 KB a workgroup stores.
// E % 64 == 0: the last block may be half (64 columns), its weight rows clamped and its second column block not stored.
// Rows past M are computed on the clamped last row and never stored.
struct FoldQueryArgs {
  const void* X; RowView xv;   // query-side hidden state, row view over the M compact rows (K = H contiguous)
  const void* Wq;              // W_cq [heads * 64][H]
  const float* bq;             // [heads * 64] or nullptr
  const void* Wk;              // per head [E][64]
  void* QP;                    // Q' [M / Q][heads * Q][E]
  int M, H, E, Q, heads, mtiles, blocks_per_slice;
};

template <typename T>
__global__ void __launch_bounds__(256) fold_query_kernel(const FoldQueryArgs a) {
  constexpr int ROWB = 128, TM = 128, NT = 256;
  constexpr int QH_BYTES = TM * ROWB;                 // Q_h tile
  constexpr int BUF1 = (64 + TM) * ROWB;              // phase 1: one K step of W_cq,h (64 rows) and X (128 rows)
  constexpr int WK_BYTES = 128 * ROWB, WK_GROUP = 3;  // phase 2: one block of W_k,h; blocks resident at a time
  constexpr int P1 = QH_BYTES, WK0 = QH_BYTES, OUT = QH_BYTES + WK_GROUP * WK_BYTES;   // phase 1's buffers lie where phase 2 keeps W_k,h (behind a barrier)
  static_assert(2 * BUF1 <= WK_GROUP * WK_BYTES, "phase 1 fits in what phase 2 uses");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using V8 = typename Vec8<T>::type;
  using V4 = typename Vec4<T>::type;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int mt = blockIdx.x % a.mtiles, rest = blockIdx.x / a.mtiles;
  const int head = rest % a.heads, slice = rest / a.heads;
  const int m0 = mt * TM, M = a.M, H = a.H, E = a.E;
  const int lm = lane & 15, ln = (lane >> 4) * 4;

  // ---- phase 1 ----
  const char* srcW[2];
  const char* srcX[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int q = tid + i * NT;
    const int row = q >> 3, c = (q & 7) ^ ((row >> 1) & 7);
    srcW[i] = (const char*)a.Wq + ((long long)(head * 64 + row) * H + c * 8) * 2;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = tid + i * NT;
    const int row = q >> 3, c = (q & 7) ^ ((row >> 1) & 7);
    const int m = min(m0 + row, M - 1);
    const int item = m / a.xv.rpi, r = m - item * a.xv.rpi;
    srcX[i] = (const char*)a.X + ((long long)item * a.xv.item_stride + (long long)r * a.xv.ld + c * 8) * 2;
  }
  const int wave_q0 = wave * 64;
  auto stage1 = [&](int buf, int kt) {
    char* base = smem + P1 + buf * BUF1;
    const long long koff = (long long)kt * ROWB;
#pragma unroll
    for (int i = 0; i < 2; ++i) glds16(srcW[i] + koff, base + (wave_q0 + i * NT) * 16);
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(srcX[i] + koff, base + 64 * ROWB + (wave_q0 + i * NT) * 16);
  };
  int foff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) foff[ks] = lm * ROWB + (((4 * ks + (lane >> 4)) ^ ((lm >> 1) & 7)) << 4);
  {
    const int wn0 = (wave >> 1) * 32, wm0 = (wave & 1) * 64;   // 2 x 2 waves, 32 weight rows x 64 activation rows each
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 bv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      bv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (a.bq) bv[i] = *reinterpret_cast<const f32x4*>(a.bq + head * 64 + wn0 + i * 16 + ln);
    }
    const int nk = H / 64;
    stage1(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (kt + 1 < nk) stage1((kt + 1) & 1, kt + 1);
      const char* wb = smem + P1 + (kt & 1) * BUF1 + wn0 * ROWB;
      const char* xb = smem + P1 + (kt & 1) * BUF1 + 64 * ROWB + wm0 * ROWB;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        V8 wa[2], xa[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) wa[i] = lds_read8<T>(wb + i * 16 * ROWB + foff[ks]);
#pragma unroll
        for (int j = 0; j < 4; ++j) xa[j] = lds_read8<T>(xb + j * 16 * ROWB + foff[ks]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = mfma16<T>(wa[i], xa[j], acc[i][j]);
      }
    }
    // Q_h[m][d .. d + 3] -> the activation tile of phase 2 (its own 16 KB: no barrier needed against phase 1's reads)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int d = wn0 + i * 16 + ln;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ml = wm0 + j * 16 + lm;
        const f32x4 v = acc[i][j] + bv[i];
        V4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(v[e]);
        *reinterpret_cast<V4*>(smem + ml * ROWB + (((d >> 3) ^ ((ml >> 1) & 7)) << 4) + (d & 4) * 2) = o;
      }
    }
  }
  __syncthreads();   // phase 1's buffers are dead, Q_h is complete

  // ---- phase 2 ----
  // wave w owns rows 32 w .. 32 w + 31 of the tile against every column: its Q_h fragments stay in registers, its 32 x 64 staging area is its
  // own, so from here on the waves meet only where a group of W_k,h blocks is exchanged
  const int nblk = (E + 127) / 128;
  const int b0 = slice * a.blocks_per_slice, b1 = min(b0 + a.blocks_per_slice, nblk);
  if (b0 >= b1) return;   // (workgroup-uniform)
  const char* wk = (const char*)a.Wk + (long long)head * E * 64 * 2;
  int wrow[4], wchunk[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = tid + i * NT;
    wrow[i] = q >> 3;
    wchunk[i] = ((q & 7) ^ ((wrow[i] >> 1) & 7)) * 16;
  }
  const int wm0 = wave * 32;
  V8 xa[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int j = 0; j < 2; ++j) xa[ks][j] = lds_read8<T>(smem + (wm0 + j * 16) * ROWB + foff[ks]);
  // copy-out: lane l moves chunk l & 7 of rows (l >> 3) + 8 u of the wave's 32
  long long rowoff[4];
  bool live[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int row = (lane >> 3) + u * 8;
    const int m = m0 + wm0 + row;
    live[u] = m < M;
    const int mc = live[u] ? m : M - 1;
    const int item = mc / a.Q, qq = mc - item * a.Q;
    rowoff[u] = (((long long)item * a.heads + head) * a.Q + qq) * E + ((lane & 7) ^ (row & 7)) * 8;
  }
  char* st = smem + OUT + wave * (32 * 128);
  for (int g0 = b0; g0 < b1; g0 += WK_GROUP) {
    const int g1 = min(g0 + WK_GROUP, b1);
    if (g0 > b0) __syncthreads();   // every wave is done with the previous group's blocks
    for (int blk = g0; blk < g1; ++blk) {
      char* base = smem + WK0 + (blk - g0) * WK_BYTES;
#pragma unroll
      for (int i = 0; i < 4; ++i) glds16(wk + (long long)min(blk * 128 + wrow[i], E - 1) * ROWB + wchunk[i], base + (wave_q0 + i * NT) * 16);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (also drains the previous group's stores: once per group, not per block)
    __syncthreads();
    for (int hb = 2 * g0; hb < 2 * g1; ++hb) {   // 64-column half blocks
      const int nb = hb * 64;
      if (nb >= E) break;
      f32x4 acc[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      const char* wb = smem + WK0 + (hb - 2 * g0) * (64 * ROWB);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        V8 wa[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wa[i] = lds_read8<T>(wb + i * 16 * ROWB + foff[ks]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = mfma16<T>(wa[i], xa[ks][j], acc[i][j]);
      }
      // the wave's [32 rows][64 columns] as 128-byte lines (chunk index XOR row & 7), then out in 16-byte pieces: 8 whole lines per instruction
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int d = i * 16 + ln;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int ml = j * 16 + lm;
          V4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(acc[i][j][e]);
          *reinterpret_cast<V4*>(st + ml * 128 + (((d >> 3) ^ (ml & 7)) << 4) + ((d >> 2) & 1) * 8) = o;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own writes have landed (its LDS operations run in order)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const V8 val = *reinterpret_cast<const V8*>(st + (lane + u * 64) * 16);
        if (live[u]) *reinterpret_cast<V8*>((T*)a.QP + nb + rowoff[u]) = val;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... and its reads are over before the next half block overwrites the area
    }
  }
}

std::atomic<long long> g_fold_query_launches, g_fold_rowfactor_launches;

// CU count of the current device, asked once per device (256, the MI355X's, where the runtime does not say)
int device_cus() {
  static std::atomic<int> memo[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int cus = memo[dev].load(std::memory_order_relaxed);
  if (!cus) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    memo[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

}  // namespace

long long fold_rowfactor_launch_count() { return g_fold_rowfactor_launches.load(std::memory_order_relaxed); }
long long fold_query_launch_count() { return g_fold_query_launches.load(std::memory_order_relaxed); }

int launch_fold_query(const void* X, RowView xv, const void* Wq, const float* bq, const void* Wk, void* QP, int M, int H, int E, int Q, int heads,
                      int op_dtype, hipStream_t stream) {
  if (M <= 0) return 0;
  if (!X || !Wq || !Wk || !QP || H < 64 || H % 64 || E < 64 || E % 64 || Q <= 0 || M % Q || heads <= 0 || xv.rpi <= 0 || (xv.ld & 7) || (xv.item_stride & 7)) return -1;
  FoldQueryArgs a{X, xv, Wq, bq, Wk, QP, M, H, E, Q, heads, (M + 127) / 128, 0};
  // slices of E: enough workgroups for every CU of the device, not more (each repeats phase 1)
  const int nblk = (E + 127) / 128, pairs = a.mtiles * heads, cus = device_cus();
  int slices = (cus + pairs - 1) / pairs;
  if (slices > nblk) slices = nblk;
  a.blocks_per_slice = (nblk + slices - 1) / slices;
  if (a.blocks_per_slice > 3) a.blocks_per_slice = a.blocks_per_slice / 3 * 3;   // whole groups of three resident blocks
  slices = (nblk + a.blocks_per_slice - 1) / a.blocks_per_slice;
  constexpr size_t lds = 128 * 128 + 3 * 128 * 128 + 4 * 32 * 128;   // Q_h, three W_k,h blocks, a 32 x 64 staging area per wave: 80 KB
  const void* fn = op_dtype == OP_F16 ? (const void*)fold_query_kernel<f16> : (const void*)fold_query_kernel<bf16>;
  if (!ensure_lds(fn, lds)) return -3;
  const dim3 grid(pairs * slices);
  if (op_dtype == OP_F16) hipLaunchKernelGGL(fold_query_kernel<f16>, grid, dim3(256), lds, stream, a);
  else hipLaunchKernelGGL(fold_query_kernel<bf16>, grid, dim3(256), lds, stream, a);
  if (hipGetLastError() != hipSuccess) return -4;
  g_fold_query_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

int launch_softmax_rows(const float* S, long long ld_s, void* P, long long ld_p, int rows, int kv, int kvp, float scale, int op_dtype,
                        hipStream_t stream) {
  if (rows <= 0) return 0;
  if (kv <= 0 || kvp < kv || (kvp & 3) || (ld_s & 3) || (ld_p & 3) || ld_p < kvp || ld_s < kv) return -1;
  const float sl2 = scale * LOG2E_F;
  const int nv = (kvp + 1023) / 1024;   // float4 per thread that cover the padded row
#define MRA_SM(T, NV) hipLaunchKernelGGL((softmax_rows_kernel<T, NV>), dim3(rows), dim3(256), 0, stream, S, ld_s, (T*)P, ld_p, kv, kvp, sl2)
#define MRA_SM_T(T)                                                                                   \
  do {                                                                                                \
    if (nv <= 1) MRA_SM(T, 1); else if (nv <= 2) MRA_SM(T, 2); else if (nv <= 4) MRA_SM(T, 4);          \
    else if (nv <= 9) MRA_SM(T, 9); else if (nv <= 16) MRA_SM(T, 16); else MRA_SM(T, 0);               \
  } while (0)
  if (op_dtype == OP_F16) MRA_SM_T(f16); else MRA_SM_T(bf16);
#undef MRA_SM_T
#undef MRA_SM
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_fold_rowfactor(const float* stat_m, const float* stat_l, float* factors, int rows, int R, int ntiles, void* P, long long ld_p, int tile_cols,
                          int kvp, hipStream_t stream, int* hist) {
  if (rows <= 0) return 0;
  if (ntiles <= 0 || R <= 0 || R > 512 || rows % R || !P || ld_p < kvp || ntiles * tile_cols > kvp) return -1;
  if (hist)
    hipLaunchKernelGGL(fold_rowfactor_kernel<true>, dim3((rows + 3) / 4), dim3(256), 0, stream, stat_m, stat_l, factors, rows, R, ntiles,
                       (unsigned short*)P, ld_p, tile_cols, kvp, hist);
  else
    hipLaunchKernelGGL(fold_rowfactor_kernel<false>, dim3((rows + 3) / 4), dim3(256), 0, stream, stat_m, stat_l, factors, rows, R, ntiles,
                       (unsigned short*)P, ld_p, tile_cols, kvp, (int*)nullptr);
  if (hipGetLastError() != hipSuccess) return -4;
  g_fold_rowfactor_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}

int launch_softmax_rescale(void* P, long long ld_p, const float* stat_m, const float* stat_l, int rows, int ntiles, int tile_cols, int kvp,
                           int op_dtype, hipStream_t stream, int* hist) {
  if (rows <= 0) return 0;
  if (ntiles <= 0 || ntiles > 128 || (tile_cols & 7) || (kvp & 7) || (ld_p & 7) || ld_p < kvp) return -1;
#define MRA_RS(T, PR) hipLaunchKernelGGL((softmax_rescale_kernel<T, PR>), dim3(rows), dim3(256), 0, stream, (T*)P, ld_p, stat_m, stat_l, ntiles, tile_cols, kvp, hist)
  if (op_dtype == OP_F16) { if (hist) MRA_RS(f16, true); else MRA_RS(f16, false); }
  else { if (hist) MRA_RS(bf16, true); else MRA_RS(bf16, false); }
#undef MRA_RS
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_transpose_pad(const void* src, void* dst, int R, int C, int ld_d, long long src_bs, long long dst_bs, int batch, int op_dtype,
                         hipStream_t stream) {
  if (batch <= 0 || R <= 0 || C <= 0) return 0;
  if (ld_d < R || batch > 65535) return -1;
  if (C % 8 == 0 && ld_d % 8 == 0 && C >= 64 && ld_d >= 64) {
    const dim3 grid64((C + 63) / 64, (ld_d + 63) / 64, batch);
    if (op_dtype == OP_F16) hipLaunchKernelGGL(transpose_pad64_kernel<f16>, grid64, dim3(256), 0, stream, (const f16*)src, (f16*)dst, R, C, ld_d, src_bs, dst_bs);
    else hipLaunchKernelGGL(transpose_pad64_kernel<bf16>, grid64, dim3(256), 0, stream, (const bf16*)src, (bf16*)dst, R, C, ld_d, src_bs, dst_bs);
    return hipGetLastError() == hipSuccess ? 0 : -4;
  }
  const dim3 grid((C + 31) / 32, (ld_d + 31) / 32, batch), block(256);
  if (op_dtype == OP_F16) hipLaunchKernelGGL(transpose_pad_kernel<f16>, grid, block, 0, stream, (const f16*)src, (f16*)dst, R, C, ld_d, src_bs, dst_bs);
  else hipLaunchKernelGGL(transpose_pad_kernel<bf16>, grid, block, 0, stream, (const bf16*)src, (bf16*)dst, R, C, ld_d, src_bs, dst_bs);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

namespace {
// One workgroup per weight row n: w'_e = w_e g_e - mean_e(w g) in fp32, rounded once; bias_out[n] = bias_in[n] + sum_e w_e b_e.
// (Run once per weight upload, from mra_qformer_prepare.)
template <typename T, typename TW, bool KEY>
__global__ void __launch_bounds__(256) fold_ln_weight_kernel(const TW* W, int E, const float* gain, const float* ln_bias, const float* bias_in,
                                                             T* dst, float* bias_out) {
  __shared__ float red[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x;
  const TW* w = W + (long long)n * E;
  float s = 0.f, sb = 0.f;
  for (int e = tid; e < E; e += 256) {
    const float we = (float)w[e];
    s += we * gain[e];
    sb = __builtin_fmaf(we, ln_bias[e], sb);
  }
  s = wave_sum(s);
  sb = wave_sum(sb);
  if (lane == 0) { red[wave] = s; red[4 + wave] = sb; }
  __syncthreads();
  const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / (float)E;
  if (tid == 0 && bias_out) bias_out[n] = (bias_in ? bias_in[n] : 0.f) + ((red[4] + red[5]) + (red[6] + red[7]));
  for (int e = tid; e < E; e += 256) {
    const T o = from_f32<T>((float)w[e] * gain[e] - mean);
    if (KEY) dst[((long long)(n >> 6) * E + e) * 64 + (n & 63)] = o;
    else dst[(long long)n * E + e] = o;
  }
}
}  // namespace

int launch_fold_ln_weight(const void* W, int w32, int rows, int E, const float* gain, const float* ln_bias, const float* bias_in, void* dst,
                          int key_layout, float* bias_out, int op_dtype, hipStream_t stream) {
  if (rows <= 0 || E <= 0 || !W || !gain || !ln_bias || !dst || (key_layout && rows % 64)) return -1;
#define MRA_FL(T, TW, KEY) hipLaunchKernelGGL((fold_ln_weight_kernel<T, TW, KEY>), dim3(rows), dim3(256), 0, stream, (const TW*)W, E, gain, ln_bias, bias_in, (T*)dst, bias_out)
#define MRA_FL_T(T)                                                          \
  do {                                                                       \
    if (w32) { if (key_layout) MRA_FL(T, float, true); else MRA_FL(T, float, false); } \
    else { if (key_layout) MRA_FL(T, T, true); else MRA_FL(T, T, false); }   \
  } while (0)
  if (op_dtype == OP_F16) MRA_FL_T(f16); else MRA_FL_T(bf16);
#undef MRA_FL_T
#undef MRA_FL
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace mra
