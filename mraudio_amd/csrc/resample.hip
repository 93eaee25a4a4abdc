// Audio front end, the step in front of fbank.hip: band-limited resampling of the decoded waveform to BEATs' 16 kHz, with the
// channel downmix.  Replaces the resampling inside LAVIS BeatsAudioProcessor.__call__ (torchaudio's windowed-sinc `resample`: Hann
// window, lowpass_filter_width 6, rolloff 0.99).  That package is not vendored: the arithmetic is the published algorithm as restated
// by mraudio_amd/processors/audio_processors.py (resample_sinc, the dense definition; resample_table, the sparse form built here),
// which tests/test_gpu_resample.py compares this file against.
//
// With g = gcd(rate_in, rate_out), orig = rate_in / g and new = rate_out / g, output sample m = j * new + i of a clip is
//   y[m] = sum_k c[i][k] x[j * orig + off[i] + k],   x = 0 outside the clip,
// a polyphase filter with `new` phases.  Phase i keeps only its non-zero taps: the input samples within lpw * orig / base of the
// centre i * orig / new (base = min(orig, new) * rolloff), first tap off[i], at most K of them (rows are padded with zeros to K).
//
// One launch for ALL clips of a step that share rate_in.  A workgroup owns BLK consecutive output samples of one clip:
//   1. the phase table (coefficients and first taps) is copied to LDS: new x KP floats, KP = K made odd so that neighbouring threads,
//      which sit in neighbouring phases, read different banks (44.1 kHz: 160 x 35 floats);
//   2. the input span under those outputs -- ceil((BLK - 1) orig / new) + K samples, the first tap being monotone in m -- is staged
//      ONCE in LDS as the channel mean: 16-byte loads from the 16-byte-aligned groups of each channel plane (scalar at the edges of
//      the buffer), zero outside the clip, never an address outside [0, total_in);
//   3. thread t forms outputs t, t + 256, ... as an fp32 fma chain over the K taps in ascending order (a fixed order: the CPU
//      emulation of the tests repeats it) and stores them with plain coalesced dword stores inside [0, total_out).  (Four chains side
//      by side with shared coefficient reads were tried: the launch took the same time, so the plain loop stays.)
// Neighbouring threads read the staged span orig / new samples apart.  An odd stride (3 at 48 kHz) touches 32 different banks; an
// even one (2 at 32 kHz, 6 at 96 kHz) would put lanes l and l + 16 on one bank, so for even integer ratios the image keeps one pad
// word per 32 samples, which moves the upper half of the lanes to the odd banks.
// fp32 throughout, as fbank.hip: the filterbank behind it takes a logarithm of band energies, and an f16 sample would put its
// rounding noise (2^-11 relative) straight into the quiet bands the anti-alias filter has just cleared.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "mra_common.h"
#include "mra_handle.h"

using namespace mra;
using namespace mra_host;

namespace {

constexpr int BLK = 1024;                // output samples per workgroup
constexpr int NT = 256;                  // threads per workgroup
constexpr int ROW = 6;                   // int64 per clip row
constexpr int MAX_CH = 32;               // channels per clip (larger counts in the table are clamped)
constexpr int MAX_PHASES = 1024;         // new
constexpr int MAX_TAPS = 256;            // K
constexpr int MAX_TABLE = 16384;         // new * KP floats
constexpr int MAX_SPAN = 16384;          // staged samples per workgroup
constexpr double LPW = 6.0, ROLLOFF = 0.99;
constexpr size_t MAX_LDS = sizeof(float) * ((size_t)MAX_TABLE + MAX_PHASES + 4 + MAX_SPAN + MAX_SPAN / 32 + 4);
static_assert(MAX_LDS <= 160 * 1024, "one workgroup's LDS");

__global__ void __launch_bounds__(NT) resample_kernel(const float* __restrict__ wave, long long total_in, const long long* __restrict__ clips,
                                                      int n_clip, const uint4* __restrict__ table, int table_words, int orig, int nw, int K,
                                                      int KP, int span, int skew, float* __restrict__ out, long long total_out) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  // the clip of this workgroup: the last row whose first block is <= b (the rows' first blocks ascend)
  int lo = 0, hi = n_clip - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (clips[(long long)mid * ROW + 5] <= b) lo = mid; else hi = mid - 1;
  }
  const long long* row = clips + (long long)lo * ROW;
  long long first_in = row[0], n_in = row[1], ch = row[2], first_out = row[3], n_out = row[4];
  const long long fb = row[5];
  // the row, clipped: nothing outside [0, total_in) or [0, total_out) is ever addressed
  if (first_in < 0) first_in = 0;
  if (first_in > total_in) first_in = total_in;
  if (n_in < 0) n_in = 0;
  if (n_in > total_in) n_in = total_in;
  if (ch < 0) ch = 0;
  if (ch > MAX_CH) ch = MAX_CH;
  if (n_out < 0) n_out = 0;
  if (n_out > total_out) n_out = total_out;
  if (b < fb || b - fb > n_out / BLK) return;   // uniform over the workgroup
  const long long m0 = (b - fb) * BLK;
  if (m0 >= n_out) return;
  const int C = (int)ch;

  float* s_tab = lds;
  const int* s_off = (const int*)(lds + nw * KP);
  float* s_x = lds + table_words;
  for (int w = tid; w < table_words / 4; w += NT) ((uint4*)lds)[w] = table[w];

  const long long j0 = m0 / nw;
  const int i0 = (int)(m0 - j0 * nw);
  const int off0 = ((const int*)table)[nw * KP + i0];
  const long long lo_in = j0 * orig + off0;   // the clip's sample under span position 0: the first tap of output m0
  const bool aligned = ((uintptr_t)wave & 15) == 0;
  const float inv = 1.0f / (float)(C > 0 ? C : 1);
  if (C == 0)
    for (int s = tid; s < span; s += NT) s_x[s + ((s >> 5) & skew)] = 0.0f;
  for (int c = 0; c < C; ++c) {
    if (c) __syncthreads();   // the pass before wrote the sums this one reads, with another thread-to-sample mapping
    const long long abs0 = first_in + (long long)c * n_in + lo_in;   // position 0 in the buffer (may lie outside it)
    const long long a0 = abs0 & ~3LL;
    const int shift = (int)(abs0 - a0);
    for (int q = tid; 4 * q - shift < span; q += NT) {
      const long long A = a0 + 4LL * q;
      float v[4];
      if (aligned && A >= 0 && A + 3 < total_in) {
        const float4 f = *(const float4*)(wave + A);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (A + e >= 0 && A + e < total_in) ? wave[A + e] : 0.0f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int s = 4 * q - shift + e;
        if (s < 0 || s >= span) continue;
        const long long p = lo_in + s;
        const float x = (p >= 0 && p < n_in) ? v[e] : 0.0f;   // zero outside the clip, whatever the neighbour holds
        const int a = s + ((s >> 5) & skew);
        float acc = c ? s_x[a] + x : x;
        if (c == C - 1 && C > 1) acc *= inv;
        s_x[a] = acc;
      }
    }
  }
  __syncthreads();

  for (int t = tid; t < BLK; t += NT) {
    const long long m = m0 + t;
    if (m >= n_out) break;
    const int ii = i0 + t, dj = ii / nw, i = ii - dj * nw;
    int rel = dj * orig + s_off[i] - off0;   // in [0, span - K]: the first tap ceil(m orig / new - R) is monotone in m
    rel = rel < 0 ? 0 : (rel > span - K ? span - K : rel);
    const float* cp = s_tab + i * KP;
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) {
      const int a = rel + k;
      acc = fmaf(cp[k], s_x[a + ((a >> 5) & skew)], acc);
    }
    const long long idx = first_out + m;
    if (idx >= 0 && idx < total_out) out[idx] = acc;
  }
}

struct Phases {
  int orig = 1, nw = 1, K = 1, KP = 1, span = 0, skew = 0, table_words = 0;
  long long nnz = 0;
  std::vector<uint32_t> table;   // [nw][KP] float coefficients, then [nw] int first taps, padded to a multiple of 4 words
};

// the reduced rates of a pair; false for a rate <= 0
bool reduce(int32_t rate_in, int32_t rate_out, long long* orig, long long* nw) {
  if (rate_in <= 0 || rate_out <= 0) return false;
  const long long g = std::gcd((long long)rate_in, (long long)rate_out);
  *orig = rate_in / g;
  *nw = rate_out / g;
  return true;
}

// resample_table of audio_processors.py, in float64, rounded to fp32 once.  Returns an error message, or "" on success.
std::string build(int32_t rate_in, int32_t rate_out, Phases* ph) {
  long long orig_l, nw_l;
  if (!reduce(rate_in, rate_out, &orig_l, &nw_l)) return "rate_in and rate_out must be > 0";
  if (nw_l > MAX_PHASES)
    return "rate pair needs " + std::to_string(nw_l) + " filter phases (rate_out / gcd), the limit is " + std::to_string(MAX_PHASES);
  const double pi = 3.14159265358979323846;
  const int orig = (int)std::min<long long>(orig_l, 1 << 30), nw = (int)nw_l;
  std::vector<int> first(nw, 0);
  std::vector<std::vector<double>> rows(nw);
  int K = 1;
  if (orig_l == nw_l) {
    rows[0] = {1.0};   // equal rates: the input unchanged (the channel mean of it)
  } else {
    const double base = (double)std::min(orig_l, nw_l) * ROLLOFF, R = LPW * (double)orig_l / base;
    if (2.0 * R + 1.0 > MAX_TAPS)
      return "rate pair needs " + std::to_string((long long)(2.0 * R + 1.0)) + " filter taps per phase, the limit is " + std::to_string(MAX_TAPS);
    for (int i = 0; i < nw; ++i) {
      const double centre = (double)i * orig / nw;
      const int k0 = (int)std::ceil(centre - R), k1 = (int)std::floor(centre + R);
      first[i] = k0;
      for (int k = k0; k <= k1; ++k) {
        double t = (-(double)i / nw + (double)k / orig) * base;
        t = std::min(std::max(t, -LPW), LPW);
        const double w = std::cos(t * pi / LPW / 2.0), a = t * pi;
        rows[i].push_back((a == 0.0 ? 1.0 : std::sin(a) / a) * w * w * (base / orig));
      }
      K = std::max(K, k1 - k0 + 1);
    }
  }
  const int KP = K | 1;
  if ((long long)nw * KP > MAX_TABLE)
    return "rate pair needs a table of " + std::to_string((long long)nw * KP) + " coefficients, the limit is " + std::to_string(MAX_TABLE);
  const long long span = ((long long)(BLK - 1) * orig_l + nw_l - 1) / nw_l + K + 1;
  if (span > MAX_SPAN)
    return "rate pair needs " + std::to_string(span) + " input samples per block of " + std::to_string(BLK) + " outputs, the limit is " +
           std::to_string(MAX_SPAN);
  ph->orig = orig; ph->nw = nw; ph->K = K; ph->KP = KP; ph->span = (int)span;
  ph->skew = (orig % nw == 0 && (orig / nw) % 2 == 0) ? -1 : 0;   // a mask: all ones = one pad word per 32 samples
  ph->table_words = (nw * KP + nw + 3) / 4 * 4;
  ph->table.assign(ph->table_words, 0u);
  ph->nnz = 0;
  for (int i = 0; i < nw; ++i) {
    for (size_t k = 0; k < rows[i].size(); ++k) {
      const float c = (float)rows[i][k];
      static_assert(sizeof(float) == sizeof(uint32_t), "the table holds floats and ints as 32-bit words");
      memcpy(&ph->table[(size_t)i * KP + k], &c, sizeof(float));
      if (c != 0.0f) ++ph->nnz;
    }
    memcpy(&ph->table[(size_t)nw * KP + i], &first[i], sizeof(int));
  }
  return "";
}

size_t lds_bytes(const Phases& p) { return sizeof(float) * ((size_t)p.table_words + p.span + p.span / 32 + 4); }

}  // namespace

struct mra_resample {
  int device = 0;
  Phases ph;
  uint4* table = nullptr;
};

extern "C" {

int mra_resample_create(int32_t rate_in, int32_t rate_out, mra_resample** out) {
  if (!out) return fail(MRA_EINVAL, "null argument");
  *out = nullptr;
  mra_resample* h = new mra_resample();
  const std::string err = build(rate_in, rate_out, &h->ph);
  if (!err.empty()) { delete h; return fail(MRA_EINVAL, "mra_resample_create(" + std::to_string(rate_in) + ", " + std::to_string(rate_out) + "): " + err); }
  hipError_t e = hipGetDevice(&h->device);
  if (e != hipSuccess) { delete h; return fail(MRA_EHIP, std::string("hipGetDevice: ") + hipGetErrorString(e)); }
  const size_t bytes = h->ph.table.size() * sizeof(uint32_t);
  e = hipMalloc((void**)&h->table, bytes);
  if (e != hipSuccess) { delete h; return fail(MRA_ENOMEM, std::string("hipMalloc of the resampling table: ") + hipGetErrorString(e)); }
  if ((e = hipMemcpy(h->table, h->ph.table.data(), bytes, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipFuncSetAttribute((const void*)resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MAX_LDS)) != hipSuccess) {
    (void)hipFree(h->table);
    delete h;
    return fail(MRA_EHIP, std::string("upload of the resampling table: ") + hipGetErrorString(e));
  }
  *out = h;
  return MRA_OK;
}

void mra_resample_destroy(mra_resample* h) {
  if (!h) return;
  if (h->table) (void)hipFree(h->table);
  delete h;
}

int64_t mra_resample_out_samples(int32_t rate_in, int32_t rate_out, int64_t n_in) {
  long long orig, nw;
  if (!reduce(rate_in, rate_out, &orig, &nw) || n_in < 0) return 0;
  const __int128 n = ((__int128)nw * n_in + orig - 1) / orig;
  return n > (__int128)INT64_MAX ? 0 : (int64_t)n;
}

int mra_resample_forward(mra_resample* h, const float* wave, int64_t total_in, const int64_t* clips, int32_t n_clip, float* out,
                         int64_t total_out, void* stream) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (total_in < 0 || total_out < 0 || n_clip < 0) return fail(MRA_EINVAL, "negative sample or clip count");
  if (n_clip == 0 || total_out == 0) return MRA_OK;
  if (!wave || !clips || !out) return fail(MRA_EINVAL, "null argument");
  // every clip takes ceil(n_out / BLK) blocks and the clips' outputs are disjoint parts of [0, total_out)
  const long long blocks = (long long)(total_out / BLK) + n_clip;
  if (blocks > 0x7fffffffLL) return fail(MRA_EINVAL, "too many output samples for one call: split the clips");
  static_assert(sizeof(long long) == sizeof(int64_t), "clips is read as long long");
  const Phases& p = h->ph;
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks), dim3(NT), lds_bytes(p), as_stream(stream), wave, (long long)total_in,
                     (const long long*)clips, (int)n_clip, (const uint4*)h->table, p.table_words, p.orig, p.nw, p.K, p.KP, p.span,
                     p.skew, out, (long long)total_out);
  return hipGetLastError() == hipSuccess ? MRA_OK : fail(MRA_EHIP, "resample forward launch");
}

double mra_resample_flops(mra_resample* h, int64_t total_out) {
  if (!h || total_out <= 0) return 0.0;
  return 2.0 * (double)h->ph.nnz / h->ph.nw * (double)total_out;
}

}  // extern "C"
