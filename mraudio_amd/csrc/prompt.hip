// Row gather with a cast: what the prompt assembly in front of the attached LM does to tensors (mraudio_amd/models/llm_prompt.py; reference
// models/xinstructblip.py:341-381, :541-595, there a torch.cat of ~T * (2 * modalities + 1) + 2 pieces).
//     out[i][0:width] = cast(src_s[r][0:width])      plan[i] = (s, r)
//     s == -1                       a row of +0
//     anything else out of range    a row of NaN, nothing read (the convention of a bad label in lm_head.hip)
// Forward: s picks the LM's embedding table or a modality's projection.  Backward: the same kernel with ONE source (d_embeds) and the inverse
// plan, since every projection row is used at most once.  No atomics, no LDS: an output row has one writer.
// A wave owns a row: the plan entry is read once into scalar registers, the source dtype is a wave-uniform switch, and the 64 lanes walk the
// row 8 elements each (16-byte stores, 1 KiB per wave instruction; an f32 source takes two 16-byte loads per store, an f32 output two stores
// per load).  A workgroup is 4 waves = 4 consecutive rows, so neighbouring output rows leave from one CU.  width % 8 == 0: a lane's group of
// 8 is whole or absent.
#include "kernels.h"
#include "mra_common.h"

namespace mra {
namespace {

typedef float f32x8 __attribute__((ext_vector_type(8)));

struct GatherSrcs {
  const void* ptr[GATHER_MAX_SRC];
  long long ld[GATHER_MAX_SRC];
  int rows[GATHER_MAX_SRC];
  int dtype[GATHER_MAX_SRC];   // 0 / 1 / 2 = f32 / f16 / bf16
  int n;
};

// entry s of a kernel-argument array, s wave-uniform and in range: selects, so the struct stays in scalar registers (no scratch copy)
template <typename V> __device__ __forceinline__ V pick(const V (&a)[GATHER_MAX_SRC], int s) {
  V v = a[0];
#pragma unroll
  for (int k = 1; k < GATHER_MAX_SRC; ++k) v = s == k ? a[k] : v;
  return v;
}

template <typename T> struct Nan16;
template <> struct Nan16<f16> { static constexpr short bits = (short)0x7e00; };
template <> struct Nan16<bf16> { static constexpr short bits = (short)0x7fc0; };

// 8 consecutive elements of a source row, as the output type's bits
template <typename TO> __device__ __forceinline__ i16x8 load8_as16(const void* row, int dtype, int c) {
  if (dtype == 0) {
    const float4 a = *reinterpret_cast<const float4*>(static_cast<const float*>(row) + c);
    const float4 b = *reinterpret_cast<const float4*>(static_cast<const float*>(row) + c + 4);
    i16x8 v;
    v[0] = __builtin_bit_cast(short, from_f32<TO>(a.x)); v[1] = __builtin_bit_cast(short, from_f32<TO>(a.y));
    v[2] = __builtin_bit_cast(short, from_f32<TO>(a.z)); v[3] = __builtin_bit_cast(short, from_f32<TO>(a.w));
    v[4] = __builtin_bit_cast(short, from_f32<TO>(b.x)); v[5] = __builtin_bit_cast(short, from_f32<TO>(b.y));
    v[6] = __builtin_bit_cast(short, from_f32<TO>(b.z)); v[7] = __builtin_bit_cast(short, from_f32<TO>(b.w));
    return v;
  }
  return *reinterpret_cast<const i16x8*>(static_cast<const short*>(row) + c);   // the same 16-bit type (checked on the host): a bit copy
}

template <typename TO>
__global__ __launch_bounds__(256) void gather_rows16_kernel(TO* __restrict__ out, long long ldo, int n_rows, int width, GatherSrcs srcs,
                                                            const int2* __restrict__ plan) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long i = (long long)blockIdx.x * 4 + wave;
  if (i >= n_rows) return;
  const int2 e = plan[i];
  const int s = __builtin_amdgcn_readfirstlane(e.x), r = __builtin_amdgcn_readfirstlane(e.y);
  short* o = reinterpret_cast<short*>(out) + i * ldo;
  const bool zero = s == -1;
  const bool ok = s >= 0 && s < srcs.n && r >= 0 && r < pick(srcs.rows, s);
  if (!ok) {
    const short f = zero ? (short)0 : Nan16<TO>::bits;
    const i16x8 v = {f, f, f, f, f, f, f, f};
    for (int c = lane * 8; c < width; c += 512) *reinterpret_cast<i16x8*>(o + c) = v;
    return;
  }
  const int dt = pick(srcs.dtype, s);
  const char* row = static_cast<const char*>(pick(srcs.ptr, s)) + (long long)r * pick(srcs.ld, s) * (dt == 0 ? 4 : 2);
  for (int c = lane * 8; c < width; c += 512) *reinterpret_cast<i16x8*>(o + c) = load8_as16<TO>(row, dt, c);
}

__global__ __launch_bounds__(256) void gather_rows32_kernel(float* __restrict__ out, long long ldo, int n_rows, int width, GatherSrcs srcs,
                                                            const int2* __restrict__ plan) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long i = (long long)blockIdx.x * 4 + wave;
  if (i >= n_rows) return;
  const int2 e = plan[i];
  const int s = __builtin_amdgcn_readfirstlane(e.x), r = __builtin_amdgcn_readfirstlane(e.y);
  float* o = out + i * ldo;
  const bool zero = s == -1;
  const bool ok = s >= 0 && s < srcs.n && r >= 0 && r < pick(srcs.rows, s);
  if (!ok) {
    const float f = zero ? 0.f : __builtin_nanf("");
    const float4 v = {f, f, f, f};
    for (int c = lane * 8; c < width; c += 512) {
      *reinterpret_cast<float4*>(o + c) = v;
      *reinterpret_cast<float4*>(o + c + 4) = v;
    }
    return;
  }
  const int dt = pick(srcs.dtype, s);
  const char* row = static_cast<const char*>(pick(srcs.ptr, s)) + (long long)r * pick(srcs.ld, s) * (dt == 0 ? 4 : 2);
  for (int c = lane * 8; c < width; c += 512) {
    float4 a, b;
    if (dt == 0) {
      a = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(row) + c);
      b = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(row) + c + 4);
    } else {
      const i16x8 v = *reinterpret_cast<const i16x8*>(reinterpret_cast<const short*>(row) + c);
      f32x8 x;
      if (dt == 1) {
        x = __builtin_convertvector(__builtin_bit_cast(Vec8<f16>::type, v), f32x8);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = __builtin_bit_cast(float, (unsigned)(unsigned short)v[j] << 16);
      }
      a = {x[0], x[1], x[2], x[3]};
      b = {x[4], x[5], x[6], x[7]};
    }
    *reinterpret_cast<float4*>(o + c) = a;
    *reinterpret_cast<float4*>(o + c + 4) = b;
  }
}

}  // namespace

int launch_gather_rows(void* out, long long ldo, int out_dtype, int n_rows, int width, const void* const* src_ptr, const long long* src_ld,
                       const int* src_rows, const int* src_dtype, int n_src, const int* plan, hipStream_t stream) {
  if (n_rows <= 0) return 0;
  if (n_src < 1 || n_src > GATHER_MAX_SRC || width <= 0 || width % 8 || ldo < width) return -1;
  GatherSrcs s{};
  s.n = n_src;
  for (int k = 0; k < n_src; ++k) {
    s.ptr[k] = src_ptr[k];
    s.ld[k] = src_ld[k];
    s.rows[k] = src_rows[k];
    s.dtype[k] = src_dtype[k];
  }
  const dim3 grid((n_rows + 3) / 4), block(256);
  const int2* p = reinterpret_cast<const int2*>(plan);
  if (out_dtype == 0)
    hipLaunchKernelGGL(gather_rows32_kernel, grid, block, 0, stream, (float*)out, ldo, n_rows, width, s, p);
  else if (out_dtype == 1)
    hipLaunchKernelGGL(gather_rows16_kernel<f16>, grid, block, 0, stream, (f16*)out, ldo, n_rows, width, s, p);
  else
    hipLaunchKernelGGL(gather_rows16_kernel<bf16>, grid, block, 0, stream, (bf16*)out, ldo, n_rows, width, s, p);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace mra
