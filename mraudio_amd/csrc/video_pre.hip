// Video front end, the step in front of vit.hip: the decoded uint8 frames of a step -> the normalised [n, 3, size, size] pixels
// mra_vit_forward reads, with the training transform's crop, resize and flip.  Replaces the host work of LAVIS
// AlproVideoTrainProcessor.transform / AlproVideoEvalProcessor.transform (random resized crop of the whole clip, bicubic; horizontal
// flip; ToUint8; / 255; Normalize) and the two host permutes behind them.  The arithmetic is that of
// mraudio_amd/processors/alpro_processors.py (crop_resize_table, preprocess_frames_ref: the float64 definition, pinned there to
// torch's bicubic interpolate), which tests/test_gpu_video_pre.py compares this file against.
//
// Output pixel (oy, ox) of channel c of a frame, with the clip's table row (idx_y, w_y, idx_x, w_x: four taps per output row and per
// output column, indices absolute in the source frame and already clamped to the crop box) and x = flip ? size - 1 - ox : ox:
//   v_k = sum_j w_y[oy][j] p[idx_y[oy][j]][idx_x[x][k]][c]   (k = 0 .. 3; an fp32 fma chain over j ascending, from 0)
//   h   = sum_k w_x[x][k] v_k                                  (an fp32 fma chain over k ascending, from 0)
//   q   = quantize ? floor(min(max(h, 0), 255)) : h            (the reference's ToUint8, with the clamp its bare cast leaves undefined)
//   out = (q / 255 - mean_c) / std_c                           (two IEEE divisions, as the host processor: never a pre-multiplied scale)
// fp32 throughout; the only narrowing is the optional f16 conversion at the store.  The fixed order is what the CPU emulation of the
// tests repeats.
//
// One launch for ALL frames of a step, whatever their source sizes.  A workgroup owns BAND output rows of one frame, all three
// channels.  Two forms, chosen per workgroup (uniformly) and bit-identical:
//   LDS form, when the crop is at most `size` columns wide and the band's taps span at most RAW_ROWS source rows (no downscale: what
//   a 0.9 .. 1.0-area crop of frames decoded at the model's size gives, and the identity of the eval processor):
//     1. the source rows under the band -- interleaved RGB bytes, rows of 3 W bytes, so unaligned in general -- are copied to LDS in
//        16-byte groups from the 16-byte-aligned address at or below each row's first byte (the row then starts `shift` bytes into its
//        LDS row); a group that is not wholly inside [0, src_bytes) is assembled from guarded byte loads, zero outside;
//     2. the vertical pass: a lane per crop column, for every (row of the band, channel) an fp32 chain over the four source rows,
//        written to a planar fp32 image in LDS whose column c sits at c + (c >> 3): lanes that own 8 columns each then read 32
//        different banks;
//     3. the horizontal pass: a lane forms 8 neighbouring outputs of one row, channel after channel, out of that image and stores
//        each eight as 16 bytes (f16) or 2 x 16 bytes (f32).  The x table is brought to LDS once per workgroup (tap positions as
//        offsets into the image, weights, the flip applied; entry ox at ox + (ox >> 3), so that the lanes' 16-byte reads of their
//        8 entries spread over all banks) and a lane keeps its 8 entries in registers across the three channels.
//   Gather form, otherwise (a downscaling crop, or `form` 1 of the debug entry, the comparison of tools/bench_video_frontend.py): the
//   same lane-to-output mapping and the same two chains, with the 16 taps of an output read straight from global memory.
// Measured at 1024 frames of 224 x 224 (profiles/video_frontend_line.json): see README.md.
// Every source byte is addressed through one guarded helper: nothing outside [0, src_bytes) is read, and a workgroup writes only the
// band of the frame it owns, so nothing outside `out`.  No atomics, no inline assembly, no scratch.
#include <cmath>
#include <cstdint>
#include <string>

#include "mra_common.h"
#include "mra_handle.h"

using namespace mra;
using namespace mra_host;

namespace {

constexpr int NT = 256;                  // threads per workgroup
constexpr int BAND = 8;                  // output rows per workgroup (divides size: size is a multiple of 8)
constexpr int ROW = 5;                   // int64 per output frame
constexpr int RAW_ROWS = BAND + 4;       // source rows the LDS form stages (an identity band needs BAND + 3)
constexpr int MAX_SIZE = 768;            // the largest output size the LDS plan holds
constexpr int MAX_SRC = 32767;           // source height / width: tap indices are int16

__host__ __device__ constexpr int raw_pitch(int size) { return (3 * size + 30 + 15) / 16 * 16; }   // shift <= 15, and one whole group more
__host__ __device__ constexpr int v_pitch(int size) { return size + size / 8 + 1; }
__host__ __device__ constexpr size_t lds_bytes(int size) {
  return (size_t)RAW_ROWS * raw_pitch(size) + sizeof(float) * BAND * 3 * (size_t)v_pitch(size) + 2 * 16 * (size_t)v_pitch(size) +
         2 * sizeof(float) * BAND * 4;
}
static_assert(lds_bytes(MAX_SIZE) <= 160 * 1024, "one workgroup's LDS");

struct Norm { float mean[3], std[3]; };

// byte `at` of the source buffer, 0 outside it
__device__ __forceinline__ float src_byte(const uint8_t* __restrict__ src, long long src_bytes, long long at) {
  return (at >= 0 && at < src_bytes) ? (float)src[at] : 0.0f;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename OutT>
__global__ void __launch_bounds__(NT) video_frames_kernel(const uint8_t* __restrict__ src, long long src_bytes, const long long* __restrict__ frames,
                                                          int n_out, const short* __restrict__ tap_idx, const float* __restrict__ tap_w, int n_tab,
                                                          int size, Norm nm, int quantize, int form, OutT* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int bands = size / BAND;
  const int f = blockIdx.x / bands, r0 = (blockIdx.x - f * bands) * BAND;
  if (f >= n_out) return;
  const long long* row = frames + (long long)f * ROW;
  const long long off = (row[0] < 0 || row[0] > src_bytes) ? src_bytes : row[0];   // a frame that starts outside the buffer reads as zeros
  // the row, clipped: the table row exists, the frame is at most MAX_SRC x MAX_SRC, every tap lies inside the frame
  const int H = (int)(row[1] < 1 ? 1 : (row[1] > MAX_SRC ? MAX_SRC : row[1]));
  const int W = (int)(row[2] < 1 ? 1 : (row[2] > MAX_SRC ? MAX_SRC : row[2]));
  const long long tab = row[3] < 0 ? 0 : (row[3] >= n_tab ? n_tab - 1 : row[3]);
  const bool flip = row[4] != 0;
  const short* ty = tap_idx + tab * 2 * size * 4;
  const short* tx = ty + size * 4;
  const float* wy = tap_w + tab * 2 * size * 4;
  const float* wx = wy + size * 4;

  const int xlo = clampi(tx[0], 0, W - 1), xhi = clampi(tx[(size - 1) * 4 + 3], 0, W - 1);
  const int ylo = clampi(ty[r0 * 4], 0, H - 1), yhi = clampi(ty[(r0 + BAND - 1) * 4 + 3], 0, H - 1);
  const int cw = xhi - xlo + 1, nr = yhi - ylo + 1;
  const bool staged = form == 0 && cw >= 1 && cw <= size && nr >= 1 && nr <= RAW_ROWS;   // uniform over the workgroup

  const int rp = raw_pitch(size), vp = v_pitch(size);
  uint8_t* s_raw = lds;
  float* s_v = (float*)(lds + (size_t)RAW_ROWS * rp);
  int4* s_cx = (int4*)(s_v + BAND * 3 * vp);      // per output column, at ox + (ox >> 3): where its four taps sit (a word of s_v's row, or a byte of the source row)
  float4* s_wx = (float4*)(s_cx + vp);            // ... and their weights; the flip is applied here, once
  int* s_rb = (int*)(s_wx + vp);                  // [BAND][4]: where tap row j of band row r starts in s_raw
  float* s_wy = (float*)(s_rb + BAND * 4);        // [BAND][4]

  for (int ox = tid; ox < size; ox += NT) {
    const int x = flip ? size - 1 - ox : ox;
    const short4 ik = *(const short4*)(tx + x * 4);
    const int ix[4] = {ik.x, ik.y, ik.z, ik.w};
    int at[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = clampi(ix[k], xlo, xhi) - xlo;
      at[k] = staged ? c + (c >> 3) : clampi(ix[k], 0, W - 1) * 3;
    }
    s_cx[ox + (ox >> 3)] = make_int4(at[0], at[1], at[2], at[3]);
    s_wx[ox + (ox >> 3)] = *(const float4*)(wx + x * 4);
  }

  if (staged) {
    // 1. the source rows ylo .. yhi, columns xlo .. xhi, as 16-byte groups from the aligned address at or below each row's first byte
    const int cq = (3 * cw + 30) / 16;
    for (int t = tid; t < nr * cq; t += NT) {
      const int rr = t / cq, q = t - rr * cq;
      const long long g0 = off + ((long long)(ylo + rr) * W + xlo) * 3;
      const int sh = (int)(((uintptr_t)src + (uintptr_t)g0) & 15);
      const long long at = g0 - sh + 16LL * q;
      uint4 v;
      if (at >= 0 && at + 16 <= src_bytes) {
        v = *(const uint4*)(src + at);
      } else {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e)
          if (at + e >= 0 && at + e < src_bytes) w[e >> 2] |= (uint32_t)src[at + e] << (8 * (e & 3));
        v = make_uint4(w[0], w[1], w[2], w[3]);
      }
      *(uint4*)(s_raw + (size_t)rr * rp + 16 * q) = v;
    }
    if (tid < BAND * 4) {
      const int y = clampi(ty[r0 * 4 + tid], ylo, yhi);
      const long long g0 = off + ((long long)y * W + xlo) * 3;
      s_rb[tid] = (y - ylo) * rp + (int)(((uintptr_t)src + (uintptr_t)g0) & 15);
      s_wy[tid] = wy[r0 * 4 + tid];
    }
    __syncthreads();
    // 2. the vertical pass into the planar fp32 image: a lane per crop column, the band's rows and channels in turn (their tap rows and
    //    weights are the same for every lane)
    for (int r = 0; r < BAND; ++r) {
      float wj[4];
      int rb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { wj[j] = s_wy[r * 4 + j]; rb[j] = s_rb[r * 4 + j]; }
      for (int c = tid; c < cw; c += NT) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          float acc = 0.0f;
#pragma unroll
          for (int j = 0; j < 4; ++j) acc = fmaf(wj[j], (float)s_raw[rb[j] + 3 * c + ch], acc);
          s_v[(r * 3 + ch) * vp + c + (c >> 3)] = acc;
        }
      }
    }
  }
  __syncthreads();

  // 3. the horizontal pass: 8 neighbouring outputs of one row per lane, its three channels in turn over the same taps
  const int groups = size / 8;
  for (int t = tid; t < BAND * groups; t += NT) {
    const int r = t / groups, xg = t - r * groups;
    const int oy = r0 + r;
    int4 cx[8];
    float4 wk[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      cx[e] = s_cx[xg * 9 + e];        // ox + (ox >> 3) with ox = 8 xg + e
      wk[e] = s_wx[xg * 9 + e];
    }
    float wj[4];
    long long rowat[4];
    if (!staged) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wj[j] = wy[oy * 4 + j];
        rowat[j] = off + (long long)clampi(ty[oy * 4 + j], 0, H - 1) * W * 3;
      }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float* vrow = s_v + (r * 3 + ch) * vp;
      float res[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int at[4] = {cx[e].x, cx[e].y, cx[e].z, cx[e].w};
        const float wv[4] = {wk[e].x, wk[e].y, wk[e].z, wk[e].w};
        float h = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float v;
          if (staged) {
            v = vrow[at[k]];
          } else {
            v = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) v = fmaf(wj[j], src_byte(src, src_bytes, rowat[j] + at[k] + ch), v);
          }
          h = fmaf(wv[k], v, h);
        }
        if (quantize) h = floorf(fminf(fmaxf(h, 0.0f), 255.0f));
        res[e] = (h / 255.0f - nm.mean[ch]) / nm.std[ch];
      }
      OutT* dst = out + (((long long)f * 3 + ch) * size + oy) * size + xg * 8;
      if constexpr (sizeof(OutT) == 2) {
        typename Vec8<OutT>::type o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (OutT)res[e];
        *(typename Vec8<OutT>::type*)dst = o;
      } else {
        *(float4*)dst = make_float4(res[0], res[1], res[2], res[3]);
        *(float4*)(dst + 4) = make_float4(res[4], res[5], res[6], res[7]);
      }
    }
  }
}

int frames_forward(const void* src, int64_t src_bytes, const int64_t* frames, int32_t n_out, const int16_t* tap_idx, const float* tap_w,
                   int32_t n_tab, int32_t size, const float* mean3, const float* std3, int32_t quantize, void* out, int32_t out_dtype,
                   int32_t form, void* stream) {
  if (n_out < 0 || src_bytes < 0) return fail(MRA_EINVAL, "mra_video_frames_forward: negative frame or byte count");
  if (out_dtype != MRA_F32 && out_dtype != MRA_F16) return fail(MRA_EINVAL, "mra_video_frames_forward: out_dtype must be MRA_F32 or MRA_F16");
  if (quantize != MRA_VIDEO_QUANT_NONE && quantize != MRA_VIDEO_QUANT_FLOOR)
    return fail(MRA_EINVAL, "mra_video_frames_forward: quantize must be MRA_VIDEO_QUANT_NONE (0) or MRA_VIDEO_QUANT_FLOOR (1)");
  if (form != 0 && form != 1) return fail(MRA_EINVAL, "mra_debug_video_frames_forward: form must be 0 (automatic) or 1 (gather)");
  if (size <= 0 || size % 8 != 0 || size > MAX_SIZE)
    return fail(MRA_EINVAL, "mra_video_frames_forward: size " + std::to_string(size) + " must be a positive multiple of 8, at most " +
                                std::to_string(MAX_SIZE) + " (the output rows and crop columns one workgroup keeps in LDS)");
  if (!mean3 || !std3) return fail(MRA_EINVAL, "mra_video_frames_forward: null mean / std");
  for (int c = 0; c < 3; ++c)
    if (!(std3[c] > 0.0f) || !std::isfinite(std3[c]) || !std::isfinite(mean3[c]))
      return fail(MRA_EINVAL, "mra_video_frames_forward: std must be > 0 and mean / std finite");
  if (n_out == 0) return MRA_OK;
  if (!src || !frames || !tap_idx || !tap_w || !out) return fail(MRA_EINVAL, "mra_video_frames_forward: null argument");
  if (n_tab < 1) return fail(MRA_EINVAL, "mra_video_frames_forward: n_tab must be >= 1");
  if (((uintptr_t)tap_idx & 7) || ((uintptr_t)tap_w & 15) || ((uintptr_t)out & 15) || ((uintptr_t)frames & 7))
    return fail(MRA_EINVAL, "mra_video_frames_forward: frames and tap_idx must be 8-byte aligned, tap_w and out 16-byte aligned");
  const long long blocks = (long long)n_out * (size / BAND);
  if (blocks > 0x7fffffffLL) return fail(MRA_EINVAL, "mra_video_frames_forward: too many output rows for one call: split the frames");
  static_assert(sizeof(long long) == sizeof(int64_t), "frames is read as long long");
  Norm nm;
  for (int c = 0; c < 3; ++c) { nm.mean[c] = mean3[c]; nm.std[c] = std3[c]; }
  const size_t lds = lds_bytes(size);
  auto launch = [&](auto t) -> int {
    using T = decltype(t);
    if (lds > 48 * 1024)
      HIP_TRY(hipFuncSetAttribute((const void*)video_frames_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(MAX_SIZE)));
    hipLaunchKernelGGL(video_frames_kernel<T>, dim3((unsigned)blocks), dim3(NT), lds, as_stream(stream), (const uint8_t*)src, (long long)src_bytes,
                       (const long long*)frames, (int)n_out, (const short*)tap_idx, tap_w, (int)n_tab, (int)size, nm, (int)quantize, (int)form,
                       (T*)out);
    return hipGetLastError() == hipSuccess ? MRA_OK : fail(MRA_EHIP, "video frames forward launch");
  };
  return with_f32_f16(out_dtype, launch);
}

// torch's cubic convolution coefficients (A = -0.75) for the fraction t, taps at floor - 1 .. floor + 2
void cubic_weights(double t, double* w) {
  const double A = -0.75;
  const double x0 = t + 1.0, x1 = t, x2 = 1.0 - t, x3 = 2.0 - t;
  w[0] = ((A * x0 - 5.0 * A) * x0 + 8.0 * A) * x0 - 4.0 * A;
  w[1] = ((A + 2.0) * x1 - (A + 3.0)) * x1 * x1 + 1.0;
  w[2] = ((A + 2.0) * x2 - (A + 3.0)) * x2 * x2 + 1.0;
  w[3] = ((A * x3 - 5.0 * A) * x3 + 8.0 * A) * x3 - 4.0 * A;
}

}  // namespace

extern "C" {

int mra_video_crop_table(int32_t n_src_crop, int32_t offset, int32_t n_out, int16_t* idx, float* w) {
  if (!idx || !w) return fail(MRA_EINVAL, "mra_video_crop_table: null argument");
  if (n_src_crop <= 0 || n_out <= 0 || offset < 0) return fail(MRA_EINVAL, "mra_video_crop_table: n_src_crop and n_out must be > 0 and offset >= 0");
  if ((long long)offset + n_src_crop - 1 > MAX_SRC)
    return fail(MRA_EINVAL, "mra_video_crop_table: the crop ends at index " + std::to_string((long long)offset + n_src_crop - 1) +
                                ", tap indices are int16: the limit is " + std::to_string(MAX_SRC));
  // crop_resize_table of alpro_processors.py, in float64, the weights rounded to fp32 once
  const double scale = (double)n_src_crop / (double)n_out;
  for (int o = 0; o < n_out; ++o) {
    const double x = scale * ((double)o + 0.5) - 0.5, fl = std::floor(x);
    double wd[4];
    cubic_weights(x - fl, wd);
    for (int k = 0; k < 4; ++k) {
      long long i = (long long)fl - 1 + k;
      i = i < 0 ? 0 : (i > n_src_crop - 1 ? n_src_crop - 1 : i);
      idx[o * 4 + k] = (int16_t)(offset + i);
      w[o * 4 + k] = (float)wd[k];
    }
  }
  return MRA_OK;
}

int mra_video_frames_forward(const void* src, int64_t src_bytes, const int64_t* frames, int32_t n_out, const int16_t* tap_idx, const float* tap_w,
                             int32_t n_tab, int32_t size, const float* mean, const float* std, int32_t quantize, void* out, int32_t out_dtype,
                             void* stream) {
  return frames_forward(src, src_bytes, frames, n_out, tap_idx, tap_w, n_tab, size, mean, std, quantize, out, out_dtype, 0, stream);
}

int mra_debug_video_frames_forward(const void* src, int64_t src_bytes, const int64_t* frames, int32_t n_out, const int16_t* tap_idx,
                                   const float* tap_w, int32_t n_tab, int32_t size, const float* mean, const float* std, int32_t quantize,
                                   void* out, int32_t out_dtype, int32_t form, void* stream) {
  return frames_forward(src, src_bytes, frames, n_out, tap_idx, tap_w, n_tab, size, mean, std, quantize, out, out_dtype, form, stream);
}

double mra_video_frames_bytes(int64_t n_out, int32_t src_h, int32_t src_w, int32_t size, int32_t out_dtype) {
  if (n_out <= 0 || src_h <= 0 || src_w <= 0 || size <= 0) return 0.0;
  const double esize = out_dtype == MRA_F32 ? 4.0 : 2.0;
  return (double)n_out * (3.0 * src_h * src_w + 3.0 * esize * size * size);
}

}  // extern "C"
