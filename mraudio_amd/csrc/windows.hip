// Ranked moment proposals: the top-k maximum-excess windows of a video's fused clip logits under greedy temporal NMS.
//
// Not in the reference: its ranked window list is whatever the LLM decode writes ("[[a, b], [c, d]]", parsed by
// utils/utils.py:66-132) and eval/mr_eval.py:21-94 scores pred_relevant_windows in list order.  This build's scorer
// (score.hip) cuts one span per video; this kernel is the second, opt-in head.  The definition (include/mra.h,
// mra_windows_from_logits) is in integers so that the order is exact:
//   thr = lo + alpha * (hi - lo) in fp32 as span_kernel, q[i] = rint(x[i] * 2^20) - rint(thr * 2^20),
//   score(s, e) = sum q[s..e] = P[e + 1] - P[s], order: score desc, length asc, start asc,
//   greedy NMS: suppressed when inter > nms_thd * union against a selected window (exact in fp64).
// One 512-thread workgroup per video: P (T + 1 int64, <= 32.8 KB) and the selected list live in LDS.  A thread owns the
// starts s = tid + 512 j (at most 8, T <= 4096) and caches each start's best unsuppressed window in registers; a pick
// can only invalidate the cached windows it suppresses, so only those starts are rescanned for the next rank.  The
// block maximum goes through 64-bit wave shuffles and one LDS round.  No atomics, no global scratch.
#include "kernels.h"
#include "mra_common.h"

namespace mra {

namespace {

constexpr int WIN_THREADS = 512;
constexpr int WIN_WAVES = WIN_THREADS / 64;
constexpr int WIN_MAX_CLIPS = 4096;
constexpr int WIN_STARTS = WIN_MAX_CLIPS / WIN_THREADS;   // starts per thread
constexpr int WIN_MAX_K = 64;
constexpr long long WIN_NONE = -0x7fffffffffffffffLL - 1;   // below any score (|score| <= 2^54)

// x * 2^20 is exact in fp64; clamped to +-2^40 so that 4096 terms cannot overflow int64 (NaN clamps to -2^40)
__device__ __forceinline__ long long win_fixed(float x) {
  const double v = fmin(fmax((double)x * 1048576.0, -1099511627776.0), 1099511627776.0);
  return llrint(v);
}

// the NMS test of the definition: inclusive clip indices, the product is exact (24 bits x 13 bits)
__device__ __forceinline__ bool win_suppressed(int s, int e, int s2, int e2, double thd) {
  const int inter = max(0, min(e, e2) - max(s, s2) + 1);
  const int uni = (e - s + 1) + (e2 - s2 + 1) - inter;
  return (double)inter > thd * (double)uni;
}

// key order: higher score, then the smaller tie word ((len - 1) << 12 | start: shorter, then earlier)
__device__ __forceinline__ bool win_better(long long sc, int tie, long long bsc, int btie) {
  return sc > bsc || (sc == bsc && tie < btie);
}

__global__ void __launch_bounds__(WIN_THREADS) window_proposal_kernel(const float* logits, int clips, float alpha, int top_k,
                                                                      float nms_thd, int max_len, int* windows, float* scores,
                                                                      int* counts) {
  __shared__ long long P[WIN_MAX_CLIPS + 1];
  __shared__ long long red_sc[WIN_WAVES];
  __shared__ int red_tie[WIN_WAVES];
  __shared__ float red_hi[WIN_WAVES], red_lo[WIN_WAVES];
  __shared__ int sel_s[WIN_MAX_K], sel_e[WIN_MAX_K];
  __shared__ long long qthr_sh;
  __shared__ int n_sel, picked;

  const int v = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = clips;
  const float* x = logits + (long long)v * T;
  const int cap = max_len > 0 ? min(max_len, T) : T;
  const double thd = (double)nms_thd;

  // hi / lo as span_kernel reduces them (the argmax itself is not needed: rank 1 is a maximum-sum window)
  float hi = -INFINITY, lo = INFINITY;
  for (int i = tid; i < T; i += WIN_THREADS) {
    const float y = x[i];
    if (y > hi) hi = y;
    lo = fminf(lo, y);
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float ohi = __shfl_xor(hi, o, 64);
    if (ohi > hi) hi = ohi;
    lo = fminf(lo, __shfl_xor(lo, o, 64));
  }
  if (lane == 0) { red_hi[wave] = hi; red_lo[wave] = lo; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < WIN_WAVES; ++w) {
      if (red_hi[w] > hi) hi = red_hi[w];
      lo = fminf(lo, red_lo[w]);
    }
    const float range = hi - lo;
    float thr;
    {
#pragma clang fp contract(off)  // multiply and add rounded separately, as span_kernel and the oracle do
      const float prod = alpha * range;
      thr = lo + prod;
    }
    qthr_sh = win_fixed(thr);
    n_sel = 0;
  }
  __syncthreads();
  const long long qthr = qthr_sh;

  // exact int64 prefix sums: thread t owns clips [8 t, 8 t + 8), wave scan, then the wave totals
  {
    const int i0 = tid * WIN_STARTS;
    long long q[WIN_STARTS];
    long long sum = 0;
#pragma unroll
    for (int j = 0; j < WIN_STARTS; ++j) {
      q[j] = i0 + j < T ? win_fixed(x[i0 + j]) - qthr : 0;
      sum += q[j];
    }
    long long incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (lane == 63) red_sc[wave] = incl;
    __syncthreads();
    long long run = incl - sum;
    for (int w = 0; w < wave; ++w) run += red_sc[w];
    if (tid == 0) P[0] = 0;
#pragma unroll
    for (int j = 0; j < WIN_STARTS; ++j) {
      run += q[j];
      if (i0 + j < T) P[i0 + j + 1] = run;
    }
  }
  __syncthreads();

  // per-start cache: best unsuppressed window (score, end) of start tid + 512 j; end < 0 = none left
  long long best_sc[WIN_STARTS];
  int best_e[WIN_STARTS];
#pragma unroll
  for (int j = 0; j < WIN_STARTS; ++j) { best_sc[j] = WIN_NONE; best_e[j] = -1; }
  unsigned dirty = (1u << WIN_STARTS) - 1;   // bit j: start j must be (re)scanned
  int* const win_out = windows + (long long)v * top_k * 2;
  float* const sc_out = scores + (long long)v * top_k;

  for (int k = 0; k < top_k; ++k) {
    const int nsel = k;   // every earlier round appended exactly one window
    long long tsc = WIN_NONE;
    int ttie = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < WIN_STARTS; ++j) {
      const int s = tid + j * WIN_THREADS;
      if (s < T) {
        if (dirty & (1u << j)) {
          long long bsc = WIN_NONE;
          int be = -1;
          const long long base = P[s];
          const int e_end = min(T, s + cap);
          for (int e = s; e < e_end; ++e) {
            const long long sc = P[e + 1] - base;
            if (sc > bsc) {   // strict: the shortest window of a start wins its ties
              bool sup = false;
              for (int m = 0; m < nsel && !sup; ++m) sup = win_suppressed(s, e, sel_s[m], sel_e[m], thd);
              if (!sup) { bsc = sc; be = e; }
            }
          }
          best_sc[j] = bsc;
          best_e[j] = be;
        }
        if (best_e[j] >= 0) {
          const int tie = ((best_e[j] - s) << 12) | s;
          if (win_better(best_sc[j], tie, tsc, ttie)) { tsc = best_sc[j]; ttie = tie; }
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const long long osc = __shfl_xor(tsc, o, 64);
      const int otie = __shfl_xor(ttie, o, 64);
      if (win_better(osc, otie, tsc, ttie)) { tsc = osc; ttie = otie; }
    }
    if (lane == 0) { red_sc[wave] = tsc; red_tie[wave] = ttie; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < WIN_WAVES; ++w)
        if (win_better(red_sc[w], red_tie[w], tsc, ttie)) { tsc = red_sc[w]; ttie = red_tie[w]; }
      // rank 1 is always emitted; later ranks only while the best unsuppressed score is positive
      const bool emit = tsc != WIN_NONE && (k == 0 || tsc > 0);
      if (emit) {
        const int s = ttie & 4095, e = s + (ttie >> 12);
        sel_s[k] = s;
        sel_e[k] = e;
        win_out[2 * k] = s;
        win_out[2 * k + 1] = e;
        sc_out[k] = (float)((double)tsc * (1.0 / 1048576.0));
        n_sel = k + 1;
      }
      picked = emit ? 1 : 0;
    }
    __syncthreads();
    if (!picked) break;   // uniform: read from LDS after the barrier
    if (k + 1 < top_k) {
      const int ns = sel_s[k], ne = sel_e[k];
      dirty = 0;
#pragma unroll
      for (int j = 0; j < WIN_STARTS; ++j) {
        const int s = tid + j * WIN_THREADS;
        if (s < T && best_e[j] >= 0 && win_suppressed(s, best_e[j], ns, ne, thd)) dirty |= 1u << j;
      }
    }
    // no third barrier: red_* are read by thread 0 before the barrier above, and `picked` is rewritten only after the next
    // round's first barrier, which every thread reaches after its read here
  }

  __syncthreads();
  const int n = n_sel;
  if (tid == 0) counts[v] = n;
  for (int k = n + tid; k < top_k; k += WIN_THREADS) {   // unused slots
    win_out[2 * k] = -1;
    win_out[2 * k + 1] = -1;
    sc_out[k] = 0.f;
  }
}

}  // namespace

int launch_windows(const float* logits, int videos, int clips, float alpha, int top_k, float nms_thd, int max_len, int* windows,
                   float* scores, int* counts, hipStream_t stream) {
  if (videos <= 0) return 0;
  if (clips < 1 || clips > WIN_MAX_CLIPS || top_k < 1 || top_k > WIN_MAX_K || !(nms_thd >= 0.f && nms_thd < 1.f) || max_len < 0)
    return -1;
  hipLaunchKernelGGL(window_proposal_kernel, dim3(videos), dim3(WIN_THREADS), 0, stream, logits, clips, alpha, top_k, nms_thd,
                     max_len, windows, scores, counts);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace mra
