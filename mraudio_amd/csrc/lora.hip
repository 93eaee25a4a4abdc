// The low-rank (LoRA) branch of an adapted linear of the attached LM: replaces peft's LoraLayer as the reference configures it
// (models/model_utils.py:4-14: r = 8, lora_alpha = 8, lora_dropout = 0.05, bias "none"; applied at models/xinstructblip.py:163).
//     forward    u  = (1/q) drop(x) op(A)^T                     down    (x, A as [R][K])
//                y  = op(y0 + s u B^T)                           up_add  (B as [N][R], no mask), in place on the base product
//     backward   du = s dY op(B)                                 down    (dY, B as [N][R]: the contraction runs over N)
//                dB += s dY^T op(u)                              wgrad   (dY, u)
//                dA += (1/q) op(du)^T drop(x)                    wgrad   (x, du), the mask regenerated
//                dx = op(dx0 + (keep/q) du A)                    up_add  (A as [R][K], the mask regenerated), in place on dY W
// x [M][K], y [M][N] in the LM's 16-bit dtype, A [R][K] and B [N][R] fp32 masters, R <= 16, s = alpha / R, q = 1 - p.
// Matrix-core operands are rounded to the 16-bit dtype on their way in, accumulation is fp32; the rank-R updates are fp32 fma chains (j ascending).
// Dropout is counter based: keep(seed, m * width + k) is the lowbias32 finaliser below, so no mask is ever stored (mraudio_amd/models/lora.py
// holds the same function).  No atomics anywhere: a workgroup owns its outputs and its waves reduce through LDS in a fixed order.
#include "kernels.h"
#include "mra_common.h"

namespace mra {
namespace {

__device__ __forceinline__ bool lora_keep(unsigned long long idx, uint32_t s_lo, uint32_t s_hi, uint32_t thr) {
  uint32_t h = (uint32_t)idx ^ s_lo ^ ((uint32_t)(idx >> 32) * 0x9E3779B9u) ^ s_hi;
  h ^= h >> 16;
  h *= 0x7feb352du;
  h ^= h >> 15;
  h *= 0x846ca68bu;
  h ^= h >> 16;
  return h >= thr;   // thr = round(p 2^32): a share p of the hashes falls below it
}

template <typename T> __device__ __forceinline__ short bits_of(float v) { return __builtin_bit_cast(short, from_f32<T>(v)); }
template <typename T> __device__ __forceinline__ float float_of(short b) { return (float)__builtin_bit_cast(T, b); }
template <typename T> __device__ __forceinline__ f32x4 mfma_bits(i16x8 a, i16x8 b, f32x4 c) {
  return mfma16<T>(__builtin_bit_cast(typename Vec8<T>::type, a), __builtin_bit_cast(typename Vec8<T>::type, b), c);
}

// out[m][j] = scale * sum_k drop(X)[m][k] op(W)(j, k).  One workgroup = 16 rows; its 4 waves take the 32-wide K steps round robin
// (mfma 16x16x32, R padded to 16 with zero columns) and are summed through LDS in wave order.  K % 8 == 0: an 8-wide group of a short
// last step is either whole or absent.
template <typename T>
__global__ __launch_bounds__(256) void lora_down_kernel(const T* __restrict__ X, long long ldx, int M, int K, const float* __restrict__ W, int R,
                                                        int w_nr, float scale, uint32_t thr, uint32_t s_lo, uint32_t s_hi, float* __restrict__ out) {
  __shared__ float red[4][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  const long long m = (long long)blockIdx.x * 16 + r16;
  const bool row_ok = m < M, col_ok = r16 < R;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const int nsteps = (K + 31) / 32;
  for (int s = wave; s < nsteps; s += 4) {
    const int k = s * 32 + g * 8;
    i16x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b = {0, 0, 0, 0, 0, 0, 0, 0};
    if (k < K) {
      if (row_ok) {
        a = *reinterpret_cast<const i16x8*>(X + m * ldx + k);
        if (thr) {
          const unsigned long long base = (unsigned long long)m * (unsigned long long)K + (unsigned long long)k;
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (!lora_keep(base + j, s_lo, s_hi, thr)) a[j] = 0;
        }
      }
      if (col_ok) {
        if (!w_nr) {   // [R][K]: 8 consecutive floats
          const float4 w0 = *reinterpret_cast<const float4*>(W + (size_t)r16 * K + k);
          const float4 w1 = *reinterpret_cast<const float4*>(W + (size_t)r16 * K + k + 4);
          b[0] = bits_of<T>(w0.x); b[1] = bits_of<T>(w0.y); b[2] = bits_of<T>(w0.z); b[3] = bits_of<T>(w0.w);
          b[4] = bits_of<T>(w1.x); b[5] = bits_of<T>(w1.y); b[6] = bits_of<T>(w1.z); b[7] = bits_of<T>(w1.w);
        } else {       // [K][R]
#pragma unroll
          for (int j = 0; j < 8; ++j) b[j] = bits_of<T>(W[(size_t)(k + j) * R + r16]);
        }
      }
    }
    acc = mfma_bits<T>(a, b, acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][4 * g + r][r16] = acc[r];
  __syncthreads();
  const int row = threadIdx.x >> 4, col = threadIdx.x & 15;
  const long long mm = (long long)blockIdx.x * 16 + row;
  if (mm < M && col < R) out[mm * R + col] = scale * (((red[0][row][col] + red[1][row][col]) + red[2][row][col]) + red[3][row][col]);
}

// Y[m][n] = op(float(Y[m][n]) + scale * keep(m, n) * sum_j U[m][j] W(n, j)), in place.  A thread keeps the weights of its 8 columns in
// registers (RMAX x 8, rows past R are zero and add nothing) and walks 16 rows; one 16-byte load and store per row.
template <typename T, int RMAX>
__global__ __launch_bounds__(256) void lora_up_add_kernel(T* __restrict__ Y, long long ld, int M, int N, const float* __restrict__ U, int R,
                                                          const float* __restrict__ W, int w_nr, float scale, uint32_t thr, uint32_t s_lo,
                                                          uint32_t s_hi) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = (blockIdx.y * 64 + lane) * 8;
  const bool c_ok = c < N;   // N % 8 == 0: the 8 columns are inside together
  float w[RMAX][8];
#pragma unroll
  for (int j = 0; j < RMAX; ++j) {
#pragma unroll
    for (int e = 0; e < 8; ++e) w[j][e] = 0.f;
    if (j < R && c_ok) {
      if (w_nr) {   // [N][R]
#pragma unroll
        for (int e = 0; e < 8; ++e) w[j][e] = W[(size_t)(c + e) * R + j];
      } else {      // [R][N]
        const float4 w0 = *reinterpret_cast<const float4*>(W + (size_t)j * N + c);
        const float4 w1 = *reinterpret_cast<const float4*>(W + (size_t)j * N + c + 4);
        w[j][0] = w0.x; w[j][1] = w0.y; w[j][2] = w0.z; w[j][3] = w0.w;
        w[j][4] = w1.x; w[j][5] = w1.y; w[j][6] = w1.z; w[j][7] = w1.w;
      }
    }
  }
  const long long m0 = (long long)blockIdx.x * 64;
  for (int i = 0; i < 16; ++i) {
    const long long m = m0 + i * 4 + wave;   // wave uniform
    if (m >= M) break;
    float u[RMAX];
#pragma unroll
    for (int j = 0; j < RMAX; ++j) u[j] = j < R ? U[m * R + j] : 0.f;
    if (c_ok) {
      i16x8* p = reinterpret_cast<i16x8*>(Y + m * ld + c);
      i16x8 y = *p;
      const unsigned long long base = (unsigned long long)m * (unsigned long long)N + (unsigned long long)c;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < RMAX; ++j) acc = fmaf(u[j], w[j][e], acc);
        if (thr && !lora_keep(base + e, s_lo, s_hi, thr)) continue;   // a dropped element keeps its bits, whatever acc holds
        y[e] = bits_of<T>(fmaf(scale, acc, float_of<T>(y[e])));
      }
      *p = y;
    }
  }
}

// dW(n, j) += scale * sum_m drop(X)[m][n] op(U)[m][j].  One workgroup = 32 columns and ALL rows: its 4 waves take the 32-row steps round
// robin (two mfma 16x16x32 per step: op(U)^T, R padded to 16, against the two 16-column halves) and are summed through LDS in wave order,
// so two runs give the same bits.
template <typename T>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const T* __restrict__ X, long long ld, int M, int N, const float* __restrict__ U, int R,
                                                         float* __restrict__ dW, int dw_nr, float scale, uint32_t thr, uint32_t s_lo, uint32_t s_hi) {
  __shared__ float red[4][2][16][17];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c16 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 32;
  const short* Xb = reinterpret_cast<const short*>(X);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const int nsteps = (M + 31) / 32;
  for (int s = wave; s < nsteps; s += 4) {
    const int mb = s * 32 + g * 8;
    i16x8 a = {0, 0, 0, 0, 0, 0, 0, 0}, b0 = {0, 0, 0, 0, 0, 0, 0, 0}, b1 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long m = mb + j;
      if (m < M) {
        if (c16 < R) a[j] = bits_of<T>(U[m * R + c16]);
        const int na = n0 + c16, nb = n0 + 16 + c16;
        if (na < N && !(thr && !lora_keep((unsigned long long)m * (unsigned long long)N + (unsigned long long)na, s_lo, s_hi, thr)))
          b0[j] = Xb[m * ld + na];
        if (nb < N && !(thr && !lora_keep((unsigned long long)m * (unsigned long long)N + (unsigned long long)nb, s_lo, s_hi, thr)))
          b1[j] = Xb[m * ld + nb];
      }
    }
    acc0 = mfma_bits<T>(a, b0, acc0);
    acc1 = mfma_bits<T>(a, b1, acc1);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[wave][0][4 * g + r][c16] = acc0[r];
    red[wave][1][4 * g + r][c16] = acc1[r];
  }
  __syncthreads();
  for (int o = threadIdx.x; o < 512; o += 256) {
    // [N][R]: j fastest over the threads, [R][N]: n fastest -- neighbouring threads write neighbouring floats either way
    const int j = dw_nr ? (o & 15) : (o >> 5), cn = dw_nr ? (o >> 4) : (o & 31);
    const int n = n0 + cn, h = cn >> 4, c = cn & 15;
    if (j < R && n < N) {
      const float sum = ((red[0][h][j][c] + red[1][h][j][c]) + red[2][h][j][c]) + red[3][h][j][c];
      float* p = dw_nr ? dW + (size_t)n * R + j : dW + (size_t)j * N + n;
      *p = fmaf(scale, sum, *p);
    }
  }
}

}  // namespace

int launch_lora_down(const void* X, long long ldx, int M, int K, const float* W, int R, int w_layout, float scale, unsigned thr,
                     unsigned long long seed, float* out, int op_dtype, hipStream_t stream) {
  if (M <= 0) return 0;
  if (K <= 0 || K % 8 || R < 1 || R > 16 || ldx < K || ldx % 8 || (w_layout != LORA_NR && w_layout != LORA_RN)) return -1;
  const dim3 grid((M + 15) / 16), block(256);
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  if (op_dtype == OP_BF16)
    hipLaunchKernelGGL(lora_down_kernel<bf16>, grid, block, 0, stream, (const bf16*)X, ldx, M, K, W, R, w_layout == LORA_NR, scale, thr, lo, hi, out);
  else
    hipLaunchKernelGGL(lora_down_kernel<f16>, grid, block, 0, stream, (const f16*)X, ldx, M, K, W, R, w_layout == LORA_NR, scale, thr, lo, hi, out);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_lora_up_add(void* Y, long long ld, int M, int N, const float* U, int R, const float* W, int w_layout, float scale, unsigned thr,
                       unsigned long long seed, int op_dtype, hipStream_t stream) {
  if (M <= 0) return 0;
  if (N <= 0 || N % 8 || R < 1 || R > 16 || ld < N || ld % 8 || (w_layout != LORA_NR && w_layout != LORA_RN)) return -1;
  const dim3 grid((M + 63) / 64, (N / 8 + 63) / 64), block(256);
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  const int nr = w_layout == LORA_NR;
#define MRA_LORA_UP(T, RMAX) \
  hipLaunchKernelGGL((lora_up_add_kernel<T, RMAX>), grid, block, 0, stream, (T*)Y, ld, M, N, U, R, W, nr, scale, thr, lo, hi)
  if (op_dtype == OP_BF16) {
    if (R <= 8) MRA_LORA_UP(bf16, 8); else MRA_LORA_UP(bf16, 16);
  } else {
    if (R <= 8) MRA_LORA_UP(f16, 8); else MRA_LORA_UP(f16, 16);
  }
#undef MRA_LORA_UP
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

int launch_lora_wgrad(const void* X, long long ld, int M, int N, const float* U, int R, float* dW, int dw_layout, float scale, unsigned thr,
                      unsigned long long seed, int op_dtype, hipStream_t stream) {
  if (M <= 0) return 0;
  if (N <= 0 || N % 8 || R < 1 || R > 16 || ld < N || ld % 8 || (dw_layout != LORA_NR && dw_layout != LORA_RN)) return -1;
  const dim3 grid((N + 31) / 32), block(256);
  const uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  if (op_dtype == OP_BF16)
    hipLaunchKernelGGL(lora_wgrad_kernel<bf16>, grid, block, 0, stream, (const bf16*)X, ld, M, N, U, R, dW, dw_layout == LORA_NR, scale, thr, lo, hi);
  else
    hipLaunchKernelGGL(lora_wgrad_kernel<f16>, grid, block, 0, stream, (const f16*)X, ld, M, N, U, R, dW, dw_layout == LORA_NR, scale, thr, lo, hi);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace mra
