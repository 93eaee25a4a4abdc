// Audio front end (row A1, the input side of the audio half): waveform -> normalised Kaldi log-mel filterbank, the tensor
// mra_beats_forward consumes.  Replaces LAVIS BeatsAudioProcessor.__call__ -> torchaudio.compliance.kaldi.fbank (call sites
// evaluate.py:24 and utils/trainer.py:46 of the reference).  Neither package is vendored: the arithmetic is the published algorithm
// restated by mraudio_amd/processors/audio_processors.py (kaldi_fbank / mel_banks), which stays the definition and is what
// tests/test_gpu_fbank.py compares this file against.  BEATs' arguments are constants here, not options: 16 kHz, 25 ms windows
// every 10 ms, no dither, DC-offset removal, pre-emphasis 0.97, povey window, 512-point transform, 128 mel bins from 20 Hz,
// snip_edges, then (x - 15.41663) / (2 * 6.55582).
//
// One launch for ALL temporal positions of ALL clips of a step.  A workgroup owns 128 consecutive frames of one segment:
//   1. the 20 720 samples those frames cover are staged ONCE in LDS (x 2^15, zero past the last whole frame).  Frame t is the 400
//      samples at 160 t, so the A operand of the transform is that span read with a 160-sample row stride; the image keeps one pad
//      word per 160 samples (row stride 161 words: odd, so the 32 rows of a fragment fall into 32 different banks).
//   2. the transform as a dense product on the f32-input MFMA (32x32x2, a k-ordered fp32 fma chain): [128 x 400] . [400 x 512].
//      DC removal, pre-emphasis and the window are LINEAR, so they are folded into the table on the host in float64,
//      M = (I - 11^T / 400) . P_0.97 . diag(povey) . [cos | -sin], rounded to fp32 once: the product reads raw samples.  Eight waves:
//      wave (r, c) owns frames [64 r, 64 r + 64) x bins [64 c, 64 c + 64) as 2 x 4 tiles ordered cos | sin | cos | sin, so a lane
//      holds the cosine and the sine sum of the same (frame, bin) in the same register of two accumulators.  The table is laid out
//      [k][c][bin & 31][4]: the four B values of a lane for one k are ONE 16-byte load, a half-wave reads 512 contiguous bytes.
//      The table (819 KB) is read from L2 by every workgroup: at 128 frames per workgroup that is 6.4 KB per frame, 3.4 GB per
//      524 288-frame step (the two row halves of a workgroup read the same lines at the same time).
//   3. power = cos^2 + sin^2 in registers -> LDS (over the dead sample image) -> the 128 mel triangles as the sparse sums they
//      are (at most 10 consecutive bins each) -> log(max(e, FLT_EPSILON)) -> normalise -> one 128-value row per frame.
//   4. rows past the segment's last frame are written as zero by the same launch.
// fp32 throughout (samples reach 3e4, powers 1e13 and the output is a logarithm: f16 operands would put their rounding noise
// straight into the quiet bands); the only narrowing is the optional f16 conversion at the store.
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "mra_common.h"
#include "mra_handle.h"

using namespace mra;
using namespace mra_host;

namespace {

constexpr int WIN = 400;                          // samples per frame (25 ms)
constexpr int HOP = 160;                          // frame shift (10 ms)
constexpr int NFFT = 512;                         // padded window
constexpr int NBIN = NFFT / 2;                    // bins 0..255 (the Nyquist bin carries no mel weight)
constexpr int NMEL = 128;
constexpr int TF = 128;                           // frames per workgroup
constexpr int SPAN = (TF - 1) * HOP + WIN;        // samples under one workgroup's frames
constexpr int SPAN_LDS = SPAN + SPAN / HOP + 1;   // with one pad word per 160 samples
constexpr int ROWP = HOP + 1;                     // LDS words between consecutive frames
constexpr int PPITCH = NBIN + 1;                  // LDS row pitch of the power rows (words)
constexpr int MAXW = 12;                          // bins read per mel filter (the widest triangle covers 10)
constexpr size_t LDS_BYTES = sizeof(float) * (SPAN_LDS > TF * PPITCH ? SPAN_LDS : TF * PPITCH);
constexpr float FB_MEAN = 15.41663f, FB_STD2 = (float)(2.0 * 6.55582);
static_assert(LDS_BYTES <= 160 * 1024, "one workgroup's LDS");

template <typename TO>
__global__ void __launch_bounds__(512) fbank_kernel(const float* __restrict__ wave, long long total, const long long* __restrict__ segs,
                                                    int frame_length, int tiles, const float4* __restrict__ tab,
                                                    const int* __restrict__ mstart, const float* __restrict__ mw, TO* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r = wv >> 2, c = wv & 3;
  const int seg = blockIdx.x / tiles, t0 = (blockIdx.x - seg * tiles) * TF;
  // the segment, clipped to [0, total): nothing outside it is ever addressed
  long long first = segs[2 * (long long)seg], len = segs[2 * (long long)seg + 1];
  if (len < 0) len = 0;
  if (first < 0) { len = len > -first ? len + first : 0; first = 0; }
  if (first > total) first = total;
  if (len > total - first) len = total - first;
  const long long nfr_all = len < WIN ? 0 : (len - WIN) / HOP + 1;   // snip_edges
  const int nfr = (int)(nfr_all < frame_length ? nfr_all : frame_length);
  const int rows = frame_length - t0 < TF ? frame_length - t0 : TF;  // output rows of this workgroup
  const int nvalid = nfr - t0 < 0 ? 0 : (nfr - t0 < TF ? nfr - t0 : TF);   // of which hold a frame
  TO* o = out + ((long long)seg * frame_length + t0) * NMEL;

  if (nvalid > 0) {   // uniform over the workgroup
    const float* src = wave + first + (long long)t0 * HOP;
    const int need = (nvalid - 1) * HOP + WIN;   // <= len - t0 * HOP: frame t0 + nvalid - 1 exists
    for (int s = tid; s < SPAN; s += 512) lds[s + s / HOP] = s < need ? src[s] * 32768.0f : 0.0f;
    __syncthreads();

    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    const bool live = 64 * r < nvalid;   // uniform over the wave
    if (live) {
      const int kh = lane >> 5;
      const float* ap = lds + ROWP * (64 * r + (lane & 31)) + kh;
      const float4* bp = tab + (size_t)kh * 128 + c * 32 + (lane & 31);
      float a0 = ap[0], a1 = ap[32 * ROWP];
      float4 b = bp[0];
      for (int k0 = 0; k0 < WIN; k0 += 2) {
        const int kn = k0 + 2 < WIN ? k0 + 2 : k0;               // the last step re-reads its own operands
        const int an = kn + (kn >= HOP) + (kn >= 2 * HOP);       // sample k of a frame sits k / 160 pad words further on
        const float a0n = ap[an], a1n = ap[32 * ROWP + an];
        const float4 bn = bp[(size_t)kn * 128];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b.x, acc[0][0], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b.x, acc[1][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b.y, acc[0][1], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b.y, acc[1][1], 0, 0, 0);
        acc[0][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b.z, acc[0][2], 0, 0, 0);
        acc[1][2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b.z, acc[1][2], 0, 0, 0);
        acc[0][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b.w, acc[0][3], 0, 0, 0);
        acc[1][3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b.w, acc[1][3], 0, 0, 0);
        a0 = a0n; a1 = a1n; b = bn;
      }
    }
    __syncthreads();   // every wave is done with the sample image: the power rows take its place
    if (live) {
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int f = 64 * r + 32 * rt + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            const float re = acc[rt][2 * g][e], im = acc[rt][2 * g + 1][e];
            lds[f * PPITCH + 64 * c + 32 * g + (lane & 31)] = re * re + im * im;
          }
    }
    __syncthreads();
    {   // mel sums: thread = (filter, frame mod 4); the filter's weights stay in registers
      const int m = tid & (NMEL - 1);
      const int start = mstart[m];
      float w[MAXW];
#pragma unroll
      for (int j = 0; j < MAXW; ++j) w[j] = mw[m * MAXW + j];
      for (int f = tid >> 7; f < nvalid; f += 4) {
        const float* p = lds + f * PPITCH + start;
        float e = 0.0f;
#pragma unroll
        for (int j = 0; j < MAXW; ++j) e = fmaf(w[j], p[j], e);
        const float v = (logf(fmaxf(e, FLT_EPSILON)) - FB_MEAN) / FB_STD2;
        o[f * NMEL + m] = (TO)v;
      }
    }
  }
  for (int i = nvalid * NMEL + tid; i < rows * NMEL; i += 512) o[i] = (TO)0.0f;   // the zero tail of a short segment
}

double hz_to_mel(double f) { return 1127.0 * std::log(1.0 + f / 700.0); }

}  // namespace

struct mra_fbank {
  int device = 0;
  char* arena = nullptr;
  float4* tab = nullptr;   // the folded transform table, [k][c][bin & 31][cos g0, -sin g0, cos g1, -sin g1]
  int* mstart = nullptr;   // first bin read by each mel filter
  float* mw = nullptr;     // [128][MAXW] weights from that bin on (zero where the triangle has ended)
  long long mel_nnz = 0;
};

extern "C" {

int mra_fbank_create(mra_fbank** out) {
  if (!out) return fail(MRA_EINVAL, "null argument");
  *out = nullptr;
  const double pi = 3.14159265358979323846;
  // T = diag(povey) . [cos | -sin]; P_0.97 . T; minus the column means: all in float64, as kaldi_fbank applies them
  std::vector<double> T((size_t)WIN * NFFT);
  for (int n = 0; n < WIN; ++n) {
    const double w = std::pow(0.5 - 0.5 * std::cos(2.0 * pi * n / (WIN - 1)), 0.85);
    for (int k = 0; k < NBIN; ++k) {
      const double ang = 2.0 * pi * (double)((n * k) % NFFT) / NFFT;
      T[(size_t)n * NFFT + k] = w * std::cos(ang);
      T[(size_t)n * NFFT + NBIN + k] = -w * std::sin(ang);
    }
  }
  std::vector<double> M((size_t)WIN * NFFT);
  for (int col = 0; col < NFFT; ++col) {
    double mean = 0.0;
    for (int n = 0; n < WIN; ++n) {   // y[i] = x[i] - 0.97 x[i - 1], y[0] = x[0] - 0.97 x[0]: x[n] feeds y[n] and y[n + 1]
      double v = (n == 0 ? 0.03 : 1.0) * T[(size_t)n * NFFT + col];
      if (n + 1 < WIN) v -= 0.97 * T[(size_t)(n + 1) * NFFT + col];
      M[(size_t)n * NFFT + col] = v;
      mean += v;
    }
    mean /= WIN;
    for (int n = 0; n < WIN; ++n) M[(size_t)n * NFFT + col] -= mean;
  }
  std::vector<float> tab((size_t)WIN * NFFT);
  for (int k = 0; k < WIN; ++k)
    for (int c = 0; c < 4; ++c)
      for (int j = 0; j < 32; ++j)
        for (int q = 0; q < 4; ++q) {
          const int bin = 64 * c + 32 * (q >> 1) + j;
          tab[(((size_t)k * 4 + c) * 32 + j) * 4 + q] = (float)M[(size_t)k * NFFT + (q & 1) * NBIN + bin];
        }
  // Kaldi's mel triangles (mel_banks of audio_processors.py): 20 Hz to Nyquist, 128 bins over bins 0..255
  std::vector<int> mstart(NMEL, 0);
  std::vector<float> mw((size_t)NMEL * MAXW, 0.0f);
  long long nnz = 0;
  {
    const double mel_lo = hz_to_mel(20.0), mel_hi = hz_to_mel(8000.0), delta = (mel_hi - mel_lo) / (NMEL + 1);
    for (int b = 0; b < NMEL; ++b) {
      const double left = mel_lo + b * delta, center = mel_lo + (b + 1.0) * delta, right = mel_lo + (b + 2.0) * delta;
      double wt[NBIN];
      int lo = -1, hi = -1;
      for (int k = 0; k < NBIN; ++k) {
        const double mel = 1127.0 * std::log(1.0 + (16000.0 / NFFT) * k / 700.0);
        const double up = (mel - left) / (center - left), down = (right - mel) / (right - center);
        wt[k] = std::max(std::min(up, down), 0.0);
        if (wt[k] > 0.0) { if (lo < 0) lo = k; hi = k; ++nnz; }
      }
      if (lo < 0) continue;   // a triangle narrower than the bin spacing can hold no bin: its energy is the floor
      if (hi - lo + 1 > MAXW) return fail(MRA_ESTATE, "a mel filter is wider than the kernel's register window");
      const int start = std::min(lo, NBIN - MAXW);
      mstart[b] = start;
      for (int j = 0; j < MAXW; ++j) mw[(size_t)b * MAXW + j] = (float)wt[start + j];
    }
  }
  mra_fbank* h = new mra_fbank();
  h->mel_nnz = nnz;
  hipError_t e = hipGetDevice(&h->device);
  if (e != hipSuccess) { delete h; return fail(MRA_EHIP, std::string("hipGetDevice: ") + hipGetErrorString(e)); }
  const size_t tab_b = align_up(tab.size() * sizeof(float)), st_b = align_up(mstart.size() * sizeof(int)), mw_b = align_up(mw.size() * sizeof(float));
  e = hipMalloc((void**)&h->arena, tab_b + st_b + mw_b);
  if (e != hipSuccess) { delete h; return fail(MRA_ENOMEM, std::string("hipMalloc of the filterbank tables: ") + hipGetErrorString(e)); }
  h->tab = (float4*)h->arena;
  h->mstart = (int*)(h->arena + tab_b);
  h->mw = (float*)(h->arena + tab_b + st_b);
  if ((e = hipMemcpy(h->tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(h->mstart, mstart.data(), mstart.size() * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(h->mw, mw.data(), mw.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipFuncSetAttribute((const void*)fbank_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES)) != hipSuccess ||
      (e = hipFuncSetAttribute((const void*)fbank_kernel<f16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES)) != hipSuccess) {
    (void)hipFree(h->arena);
    delete h;
    return fail(MRA_EHIP, std::string("upload of the filterbank tables: ") + hipGetErrorString(e));
  }
  *out = h;
  return MRA_OK;
}

void mra_fbank_destroy(mra_fbank* h) {
  if (!h) return;
  if (h->arena) (void)hipFree(h->arena);
  delete h;
}

int mra_fbank_forward(mra_fbank* h, const float* wave, int64_t total_samples, const int64_t* segs, int32_t n_seg, int32_t frame_length,
                      void* out, int32_t out_dtype, void* stream) {
  if (out_dtype != MRA_F32 && out_dtype != MRA_F16) return fail(MRA_EINVAL, "out_dtype must be MRA_F32 or MRA_F16");
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (total_samples < 0 || n_seg < 0 || frame_length < 0) return fail(MRA_EINVAL, "negative sample, segment or frame count");
  if (n_seg == 0 || frame_length == 0) return MRA_OK;
  if (!wave || !segs || !out) return fail(MRA_EINVAL, "null argument");
  const int tiles = (frame_length + TF - 1) / TF;
  if ((long long)n_seg * tiles > 0x7fffffffLL) return fail(MRA_EINVAL, "too many segments for one call: split them");
  const dim3 grid((unsigned)((long long)n_seg * tiles)), block(512);
  hipStream_t st = as_stream(stream);
  static_assert(sizeof(long long) == sizeof(int64_t), "segs is read as long long");
  if (out_dtype == MRA_F32)
    hipLaunchKernelGGL(fbank_kernel<float>, grid, block, LDS_BYTES, st, wave, (long long)total_samples, (const long long*)segs, (int)frame_length, tiles,
                       (const float4*)h->tab, (const int*)h->mstart, (const float*)h->mw, (float*)out);
  else
    hipLaunchKernelGGL(fbank_kernel<f16>, grid, block, LDS_BYTES, st, wave, (long long)total_samples, (const long long*)segs, (int)frame_length, tiles,
                       (const float4*)h->tab, (const int*)h->mstart, (const float*)h->mw, (f16*)out);
  return hipGetLastError() == hipSuccess ? MRA_OK : fail(MRA_EHIP, "fbank forward launch");
}

double mra_fbank_flops(mra_fbank* h, int32_t n_seg, int32_t frame_length) {
  if (!h || n_seg <= 0 || frame_length <= 0) return 0.0;
  return (double)n_seg * frame_length * (2.0 * WIN * NFFT + 3.0 * NBIN + 2.0 * (double)h->mel_nnz);
}

}  // extern "C"
