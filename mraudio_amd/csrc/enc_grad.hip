// Encoder side of the Q-Former backward (BASELINE config 5; not in the reference, whose Q-Formers are frozen,
// models/xinstructblip.py:196-204): the gradient of the training step with respect to the features the K/V projection read, and the
// backward of the modality LayerNorm in front of it.
//
//   kvgrad_gemm_kernel   dY_enc[m][e] = sum_k dKV[m][k] W_kv[k][e],  m = item * kv + tok,  k = (cl * 2 + sel) * H + head * 64 + d.
//     A is the head-major dK / dV tape [ncross * 2][Ne][heads][kv][64] read IN PLACE: the 64-wide K step s = k / 64 of row m is the 128-byte
//     row at (((s / heads) * Ne + item) * heads + s % heads) * kv * 64 + tok * 64, so inside an (item, head) block a run of tokens is one
//     contiguous stream.  A tile of 128 rows is staged per K step by LDS-DMA (four 16-byte chunks per thread; the item / token split of a row
//     is done once per thread, so a tile may straddle items) with the 16-byte chunk index XOR (row & 7) on the SOURCE address, and read
//     back with ds_read_b64 in the k order the transposed B read delivers (element j of a fragment: k = 8 (j >> 2) + 4 (lane >> 5) + (j & 3)).
//     W_kv is read as stored, [K][E], k-major -- the wrong way round for an MFMA operand: [32 k][64 e] tiles staged and read with
//     ds_read_b64_tr_b16 exactly like the X operand of gemm_tn.hip.  No transposed copy of the weights exists, so none can go stale.
//     One workgroup = 128 rows x 128 columns (4 waves, 64 x 64 each: four v_mfma_f32_32x32x16 accumulators), two LDS stages of 32 KB: the
//     next K step is in flight while this one is multiplied, one barrier per step.  fp32 out, rows past M are loaded clamped and not stored.
//     ROWS = true is the second A-side addressing mode (launch_rowgrad_gemm: the data gradient of the LLM projection, proj_grad.hip): A is a
//     plain row-major [M][K] matrix, i.e. the tape above with kv = 1 and K / 64 heads of one selector, so the per-row division and the
//     per-step selector split drop out at compile time; staging, fragment order and arithmetic are the ones above.
//   modality_ln_bwd_kernel   d_x = r (g - mean(g) - xhat mean(g xhat)), g = d_out gain; d_gain += sum_rows d_out xhat; d_bias += sum_rows d_out.
//     One wave per row, the row in registers (8 elements per lane and step, the buckets of modality_ln_kernel), statistics two-pass from
//     x.  A row is read completely before it is written, so d_x may be d_out.  Column sums meet in LDS (one fp32 LDS atomic per element
//     and row), then one global float atomic per column and workgroup.
#include "kernels.h"
#include "mra_common.h"

#include <algorithm>

namespace mra {

namespace {

constexpr int KG_BM = 128, KG_BN = 128;
constexpr int KG_A_BYTES = KG_BM * 128;            // [128 rows][64 k]
constexpr int KG_W_TILE = 32 * 128;                // [32 k][64 e]
constexpr int KG_STAGE = KG_A_BYTES + 4 * KG_W_TILE;

template <typename T, bool ROWS>
__global__ void __launch_bounds__(256) kvgrad_gemm_kernel(const T* __restrict__ dkv, const T* __restrict__ W, float* __restrict__ out, int M, int kv,
                                                           int Ne, int heads, int nseg, int E) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = blockIdx.x * KG_BM, e0 = blockIdx.y * KG_BN;

  // A: chunk idx = tid + 256 i of the tile: row idx >> 3, physical chunk idx & 7 holds source chunk (idx & 7) ^ (row & 7)
  const T* arow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = tid + 256 * i, r = idx >> 3;
    const int m = min(m0 + r, M - 1);              // rows past M: a valid row again, never stored
    const int item = ROWS ? m : m / kv, tok = ROWS ? 0 : m - item * kv;
    arow[i] = dkv + ((long long)item * heads * kv + tok) * 64 + (((idx & 7) ^ (r & 7)) << 3);
  }
  const long long head_stride = (long long)kv * 64, sel_stride = (long long)Ne * heads * kv * 64;
  // W: four [32 k][64 e] tiles per step (column half cb, k half kh), one 16-byte chunk per thread each, staged as gemm_tn.hip stages X
  const int srow = tid >> 3, sc = tid & 7;
  const T* wsrc = W + (long long)srow * E + e0 + ((sc ^ (((srow >> 1) & 1) << 2)) << 3);
  auto issue = [&](int buf, int s) {
    char* st = smem + buf * KG_STAGE;
    const int g = ROWS ? 0 : s / heads;
    const long long seg = (long long)g * sel_stride + (long long)(s - g * heads) * head_stride;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(arow[i] + seg, st + i * 4096 + wave * 1024);
    const T* wk = wsrc + (long long)s * 64 * E;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) glds16(wk + (long long)kh * 32 * E + cb * 64, st + KG_A_BYTES + (cb * 2 + kh) * KG_W_TILE + wave * 1024);
  };
  const int wm = wave >> 1, wn = wave & 1;   // this wave's 64 rows (two 32-row blocks) and 64 columns (two 32-column blocks)
  // A fragment of k16 step q (0 .. 3): chunks 2 q and 2 q + 1 of row wm * 64 + (lane & 31) (+ 32: 4096 bytes on, the same swizzle), 8 bytes at
  // 8 (lane >> 5)
  unsigned a_off[8];
  {
    const int r = wm * 64 + (lane & 31);
#pragma unroll
    for (int c = 0; c < 8; ++c) a_off[c] = r * 128 + ((c ^ (r & 7)) << 4) + ((lane >> 5) << 3);
  }
  // transposed-read lane offsets of the B fragments (derivation: gemm_tn.hip)
  unsigned b_off[2];
  {
    const int g = lane >> 4, i = lane & 15, q4 = i >> 2, p = i & 3, h = lane >> 5;
    const int row = 4 * h + q4;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int c = 4 * ct + 2 * (g & 1) + (p >> 1);
      const int pc = c ^ (((q4 >> 1) & 1) << 2);
      b_off[ct] = KG_A_BYTES + wn * 2 * KG_W_TILE + row * 128 + pc * 16 + (p & 1) * 8;
    }
  }
  const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

  f32x16 acc[2][2];   // [row block][column block]
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[0][0][i] = 0.f; acc[0][1][i] = 0.f; acc[1][0][i] = 0.f; acc[1][1][i] = 0.f; }
  issue(0, 0);
  int buf = 0;
  for (int s = 0; s < nseg; ++s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();            // step s has landed for every wave, and every wave is done reading the other stage
    asm volatile("" ::: "memory");
    if (s + 1 < nseg) issue(buf ^ 1, s + 1);
    const unsigned base = lds0 + buf * KG_STAGE;
    buf ^= 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // k16 step q of the 64: W rows 16 q .. 16 q + 15 = tile kh = q >> 1, rows 16 (q & 1) ..
      const unsigned bq = base + (q >> 1) * KG_W_TILE + (q & 1) * 2048;
      i16x4 a0, a1, a2, a3, b00, b01, b10, b11;
      asm volatile(
          "ds_read_b64 %0, %8\n\t"
          "ds_read_b64 %1, %9\n\t"
          "ds_read_b64 %2, %8 offset:4096\n\t"
          "ds_read_b64 %3, %9 offset:4096\n\t"
          "ds_read_b64_tr_b16 %4, %10\n\t"
          "ds_read_b64_tr_b16 %5, %10 offset:1024\n\t"
          "ds_read_b64_tr_b16 %6, %11\n\t"
          "ds_read_b64_tr_b16 %7, %11 offset:1024\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(a0), "=&v"(a1), "=&v"(a2), "=&v"(a3), "=&v"(b00), "=&v"(b01), "=&v"(b10), "=&v"(b11)
          : "v"(base + a_off[2 * q]), "v"(base + a_off[2 * q + 1]), "v"(bq + b_off[0]), "v"(bq + b_off[1])
          : "memory");
      auto cat = [](i16x4 lo, i16x4 hi) {
        i16x8 v8;
        v8[0] = lo[0]; v8[1] = lo[1]; v8[2] = lo[2]; v8[3] = lo[3];
        v8[4] = hi[0]; v8[5] = hi[1]; v8[6] = hi[2]; v8[7] = hi[3];
        return v8;
      };
      const auto A0 = __builtin_bit_cast(typename Vec8<T>::type, cat(a0, a1)), A1 = __builtin_bit_cast(typename Vec8<T>::type, cat(a2, a3));
      const auto B0 = __builtin_bit_cast(typename Vec8<T>::type, cat(b00, b01)), B1 = __builtin_bit_cast(typename Vec8<T>::type, cat(b10, b11));
      acc[0][0] = mfma32<T>(A0, B0, acc[0][0]);
      acc[0][1] = mfma32<T>(A0, B1, acc[0][1]);
      acc[1][0] = mfma32<T>(A1, B0, acc[1][0]);
      acc[1][1] = mfma32<T>(A1, B1, acc[1][1]);
    }
  }
  // D: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int col = e0 + wn * 64 + ct * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m < M) out[(long long)m * E + col] = acc[mb][ct][r];
      }
    }
}

// 8 consecutive elements of a row as f32
template <typename TI>
__device__ __forceinline__ void lnb_load8(const TI* p, float (&v)[8]);
template <>
__device__ __forceinline__ void lnb_load8<float>(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}
template <>
__device__ __forceinline__ void lnb_load8<f16>(const f16* p, float (&v)[8]) {
  const Vec8<f16>::type h = *reinterpret_cast<const Vec8<f16>::type*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)h[e];
}
template <>
__device__ __forceinline__ void lnb_load8<bf16>(const bf16* p, float (&v)[8]) {
  const Vec8<bf16>::type h = *reinterpret_cast<const Vec8<bf16>::type*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)h[e];
}

// rows of E (multiple of 8, <= 512 * MAXC) elements.  Wave w of workgroup b takes rows b * 4 + w, + 4 * gridDim.x, ...  Every lane loads on
// every step (a lane past the row end re-reads the last chunk and zeroes it), as modality_ln_kernel does.
template <typename TI, int MAXC>
__global__ void __launch_bounds__(256) modality_ln_bwd_kernel(const TI* x, const float* d_out, const float* gain, float eps, long long rows, int E,
                                                               float* d_x, float* d_gain, float* d_bias) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem);   // [2][E], only with a column sum
  const bool sums = d_gain != nullptr || d_bias != nullptr;
  const int lane = threadIdx.x & 63;
  const int nc = E >> 3;
  if (sums) {
    for (int c = threadIdx.x; c < 2 * E; c += 256) red[c] = 0.f;
    __syncthreads();
  }
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * 4) {
    const TI* xr = x + row * E;
    const float* dr = d_out + row * E;
    float v[MAXC][8], dy[MAXC][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = i * 64 + lane;
      const int cc = c < nc ? c : nc - 1;
      lnb_load8<TI>(xr + cc * 8, v[i]);
      lnb_load8<float>(dr + cc * 8, dy[i]);
      if (c >= nc) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[i][e] = 0.f; dy[i][e] = 0.f; }
      }
      s += ((v[i][0] + v[i][1]) + (v[i][2] + v[i][3])) + ((v[i][4] + v[i][5]) + (v[i][6] + v[i][7]));
    }
    const float mean = wave_sum(s) / (float)E;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const bool live = i * 64 + lane < nc;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[i][e] = live ? v[i][e] - mean : 0.f;
        q += v[i][e] * v[i][e];
      }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)E + eps);
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = i * 64 + lane;
      const int cc = c < nc ? c : nc - 1;
      float gm[8];
      lnb_load8<float>(gain + cc * 8, gm);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[i][e] *= rstd;   // xhat (0 on dead lanes)
        const float g = dy[i][e] * gm[e];
        sg += g;
        sgx += g * v[i][e];
        if (sums && c < nc) {
          if (d_gain) atomicAdd(&red[e * nc + c], dy[i][e] * v[i][e]);   // column c * 8 + e at [e][c]: lanes on consecutive banks
          if (d_bias) atomicAdd(&red[E + e * nc + c], dy[i][e]);
        }
        dy[i][e] = g;
      }
    }
    sg = wave_sum(sg) / (float)E;
    sgx = wave_sum(sgx) / (float)E;
    if (d_x) {   // the whole row was read above: d_x may be d_out
      float* dxr = d_x + row * E;
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        const int c = i * 64 + lane;
        f32x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          lo[e] = rstd * (dy[i][e] - sg - v[i][e] * sgx);
          hi[e] = rstd * (dy[i][4 + e] - sg - v[i][4 + e] * sgx);
        }
        if (c < nc) {
          *reinterpret_cast<f32x4*>(dxr + c * 8) = lo;
          *reinterpret_cast<f32x4*>(dxr + c * 8 + 4) = hi;
        }
      }
    }
  }
  if (!sums) return;
  __syncthreads();
  for (int c = threadIdx.x; c < E; c += 256) {
    const int at = (c & 7) * nc + (c >> 3);
    if (d_gain) unsafeAtomicAdd(d_gain + c, red[at]);
    if (d_bias) unsafeAtomicAdd(d_bias + c, red[E + at]);
  }
}

template <typename TI>
int modality_ln_bwd_t(const void* x, const float* d_out, const float* gain, float eps, long long rows, int E, float* d_x, float* d_gain,
                      float* d_bias, hipStream_t stream) {
  // at most two workgroups per compute unit: the column sums cost 2 E global atomics per workgroup
  const unsigned blocks = (unsigned)std::min<long long>((rows + 3) / 4, 512);
  const size_t lds = (d_gain || d_bias) ? (size_t)2 * E * 4 : 0;
#define MRA_LNB_CASE(MAXC)                                                                                                          \
  hipLaunchKernelGGL((modality_ln_bwd_kernel<TI, MAXC>), dim3(blocks), dim3(256), lds, stream, (const TI*)x, d_out, gain, eps, rows, E, d_x, \
                     d_gain, d_bias)
  if (E <= 1024) MRA_LNB_CASE(2);
  else if (E <= 1536) MRA_LNB_CASE(3);
  else if (E <= 4096) MRA_LNB_CASE(8);
  else return -1;
#undef MRA_LNB_CASE
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace

int launch_kvgrad_gemm(const void* dkv, const void* W, float* d_enc, int Ne, int kv, int heads, int nsel, int E, int op_dtype, hipStream_t stream) {
  if (Ne <= 0 || kv <= 0) return 0;
  if (heads <= 0 || nsel <= 0 || E <= 0 || E % KG_BN) return -1;
  const long long M = (long long)Ne * kv;
  if (M > 0x7fffffffLL - KG_BM) return -1;
  const dim3 grid((unsigned)((M + KG_BM - 1) / KG_BM), E / KG_BN), block(256);
  const size_t lds = 2 * KG_STAGE;
  if (op_dtype == OP_F16)
    hipLaunchKernelGGL((kvgrad_gemm_kernel<f16, false>), grid, block, lds, stream, (const f16*)dkv, (const f16*)W, d_enc, (int)M, kv, Ne, heads, nsel * heads, E);
  else
    hipLaunchKernelGGL((kvgrad_gemm_kernel<bf16, false>), grid, block, lds, stream, (const bf16*)dkv, (const bf16*)W, d_enc, (int)M, kv, Ne, heads, nsel * heads, E);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_rowgrad_gemm(const void* dY, const void* W, float* dX, int M, int K, int E, int op_dtype, hipStream_t stream) {
  if (M <= 0) return 0;
  if (K <= 0 || K % 64 || E <= 0 || E % KG_BN || M > 0x7fffffff - KG_BM) return -1;
  const dim3 grid((unsigned)((M + KG_BM - 1) / KG_BM), E / KG_BN), block(256);
  const size_t lds = 2 * KG_STAGE;
  // row m is "item" m of one token with K / 64 heads: the head-major address of K step s is then m * K + s * 64
  if (op_dtype == OP_F16)
    hipLaunchKernelGGL((kvgrad_gemm_kernel<f16, true>), grid, block, lds, stream, (const f16*)dY, (const f16*)W, dX, M, 1, M, K / 64, K / 64, E);
  else
    hipLaunchKernelGGL((kvgrad_gemm_kernel<bf16, true>), grid, block, lds, stream, (const bf16*)dY, (const bf16*)W, dX, M, 1, M, K / 64, K / 64, E);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_modality_ln_bwd(const void* x, int x_dtype, int items, int tokens, int E, const float* gain, float eps, const float* d_out, float* d_x,
                           float* d_gain, float* d_bias, hipStream_t stream) {
  if (items <= 0 || tokens <= 0) return 0;
  if (E % 8 || E <= 0) return -1;
  if (!d_x && !d_gain && !d_bias) return 0;
  const long long rows = (long long)items * tokens;
  if (rows > 0x7fffffffLL) return -1;
  switch (x_dtype) {
    case 0: return modality_ln_bwd_t<float>(x, d_out, gain, eps, rows, E, d_x, d_gain, d_bias, stream);
    case 1: return modality_ln_bwd_t<f16>(x, d_out, gain, eps, rows, E, d_x, d_gain, d_bias, stream);
    case 2: return modality_ln_bwd_t<bf16>(x, d_out, gain, eps, rows, E, d_x, d_gain, d_bias, stream);
  }
  return -2;
}

}  // namespace mra
