// GEMM main-loop experiments of round 1 (A/B material, NOT part of the shipped library).
// Included by gemm.hip only when MRA_GEMM_EXPERIMENTS is defined (tests/native/libmra_hip_exp.so, used by
// gemm_bench and kernel_check).  Verdicts are in DESIGN.md section 8; they stay in the tree so the
// measurements can be repeated:
//   0 ring      LDS ring of 32-deep slots, counted vmcnt               slower than the two-buffer loop
//   2 v1 + PF   L2 prefetch two tiles ahead                            slower
//   3 v1 spread LDS-DMA issue spread between MFMA groups               no gain
//   4 v1 stamp  s_memtime stamps per loop segment (diagnostic)
//   6 ws NODMA  loaders stop after tile 1 (diagnostic, wrong results)
//   7 ws2       4-slot ring, LDS counter hand-off, no K-loop barrier   slower
//   8 k128 everywhere (the shipped default uses it for K >= 2048 only)
//   9 rot       second half of each K tile deferred past the barrier, DMA interleaved
//  10 w4        9 rot on four waves of 128 x 128 (256 accumulator registers per lane, one wave per SIMD)
//  11 w4p       four waves of 128 x 128, two fragment register sets: every LDS read one half-tile ahead of its use
// =================================================================================================
// ring main loop: slots of 32 k (64-byte rows)
// =================================================================================================
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
  else static_assert(N == 0, "add the vmcnt immediate");
}

template <typename T, int TN, int TM, int WGN, int WGM, int NS, int SPI, int EPI>
__global__ void __launch_bounds__(WGN* WGM * 64) gemm_ring_kernel(const GemmArgs args) {
  constexpr int NT = WGN * WGM * 64;
  constexpr int WTN = TN / WGN, WTM = TM / WGM;
  constexpr int FN = WTN / 16, FM = WTM / 16;
  constexpr int SK = 32, SROW = SK * 2;                  // slot depth, bytes per staged row
  constexpr int IW = TN * 4 / NT, IX = TM * 4 / NT;      // 16-byte chunks per thread per operand per slot
  static_assert(TN * 4 % NT == 0 && TM * 4 % NT == 0, "tile/threads mismatch");
  static_assert(NS >= 2 * SPI, "ring too small");
  constexpr int LPS = IW + IX;                           // LDS-DMA instructions per thread per slot
  constexpr int SLOT = (TN + TM) * SROW;
  constexpr int KEEP = LPS * (NS - 2 * SPI);             // loads that may stay in flight at the wait
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn0 = (wave / WGM) * WTN;
  const int wm0 = (wave % WGM) * WTM;
  int n0, m0;
  const GemmProb& P = pick_tile<TN, TM>(args, n0, m0);
  const int K = P.K, M = P.M;

  // per-lane source pointers; physical chunk c' = q & 3 of row q >> 2 holds source chunk c' ^ ((-(row >> 2)) & 3)
  const char* srcW[IW];
  const char* srcX[IX];
#pragma unroll
  for (int i = 0; i < IW; ++i) {
    const int q = tid + i * NT;
    const int row = q >> 2, c = (q & 3) ^ ((-(row >> 2)) & 3);
    srcW[i] = (const char*)P.W + ((long long)(n0 + row) * K + c * 8) * 2;
  }
#pragma unroll
  for (int i = 0; i < IX; ++i) {
    const int q = tid + i * NT;
    const int row = q >> 2, c = (q & 3) ^ ((-(row >> 2)) & 3);
    const int m = min(m0 + row, M - 1);  // rows past M are computed on a clamped row and never stored
    srcX[i] = (const char*)P.A + (view_off(P.a, m) + c * 8) * 2;
  }
  const int wave_q0 = wave * 64;

  auto issue = [&](int slot, int t) {
    char* base = smem + slot * SLOT;
    const long long koff = (long long)t * SROW;
#pragma unroll
    for (int i = 0; i < IW; ++i) glds16(srcW[i] + koff, base + (wave_q0 + i * NT) * 16);
#pragma unroll
    for (int i = 0; i < IX; ++i) glds16(srcX[i] + koff, base + TN * SROW + (wave_q0 + i * NT) * 16);
  };

  // fragment read offset: row (lane & 15), logical chunk (lane >> 4), swizzled
  const int foff = (lane & 15) * SROW + ((((lane >> 4)) ^ ((-((lane & 15) >> 2)) & 3)) << 4);

  f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nslots = K / SK;          // host guarantees K % (SK * SPI) == 0
  const int niter = nslots / SPI;
#pragma unroll
  for (int s = 0; s < NS; ++s)
    if (s < nslots) issue(s, s);

  int cslot = 0;                      // ring position of the first slot of this iteration
  for (int it = 0; it < niter; ++it) {
    // slots it*SPI .. it*SPI+SPI-1 must have landed; younger ones may stay in flight
    if (nslots - (it + 1) * SPI >= NS - 2 * SPI) wait_vmcnt<KEEP>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");  // the raw barrier is IntrNoMem: keep LDS traffic below it
    // refill the slots iteration it-1 consumed (every wave is past its reads of them now)
    if (it >= 1) {
#pragma unroll
      for (int j = 0; j < SPI; ++j) {
        const int t = (it - 1) * SPI + NS + j;
        int rs = cslot - SPI + j;
        rs = rs < 0 ? rs + NS : rs;
        if (t < nslots) issue(rs, t);
      }
    }
#pragma unroll
    for (int j = 0; j < SPI; ++j) {
      int s = cslot + j;
      s = s >= NS ? s - NS : s;
      const char* wb = smem + s * SLOT + wn0 * SROW + foff;
      const char* xb = smem + s * SLOT + TN * SROW + wm0 * SROW + foff;
      typename Vec8<T>::type a[FN], b[FM];
#pragma unroll
      for (int i = 0; i < FN; ++i) a[i] = lds_read8<T>(wb + i * 16 * SROW);
#pragma unroll
      for (int jj = 0; jj < FM; ++jj) b[jj] = lds_read8<T>(xb + jj * 16 * SROW);
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int jj = 0; jj < FM; ++jj) acc[i][jj] = mfma16<T>(a[i], b[jj], acc[i][jj]);
      __builtin_amdgcn_s_setprio(0);
    }
    cslot += SPI;
    cslot = cslot >= NS ? cslot - NS : cslot;
  }
  if constexpr (EPI == EPI_OP || EPI == EPI_GELU_OP || EPI == EPI_KV) {
    __syncthreads();
    epilogue_lds16<T, TN, TM, FN, FM, NT, EPI>(P, acc, smem, n0, m0, wn0, wm0, tid);
  } else {
    epilogue<T, FN, FM, EPI>(P, acc, n0 + wn0, m0 + wm0, lane);
  }
}

// =================================================================================================
// v1 main loop: two 64-deep buffers (128-byte rows), vmcnt(0) + __syncthreads per K tile
// =================================================================================================
// PF: every wave also touches, two K tiles ahead of the LDS-DMA stage, the 64 cache lines of its share
// of that tile with two 4-byte LDS-DMA loads per lane-line (dummy LDS target), so that the ~22 % of
// stage loads that would miss the XCD's L2 (measured TCC hit rate 78 %) are L2 hits by the time the
// stage is issued: vmcnt retires in order, so one slow miss per stage sets the whole stage's latency.
// SPREAD: the LDS-DMA instructions of the next K tile are not issued in one burst after the barrier
// but one at a time between groups of MFMAs (an LDS-DMA issue costs 60-185 cycles of the wave's issue
// slot; in a burst both waves of a SIMD pay it at the same time and the matrix pipe idles).  The two
// waves that share a SIMD (wave w and w + 4) use opposite phases so their VMEM issues alternate.
__device__ __forceinline__ unsigned long long stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}

template <typename T, int TN, int TM, int WGN, int WGM, int EPI, bool PF, bool SPREAD = false, bool STAMP = false>
__global__ void __launch_bounds__(WGN* WGM * 64) gemm_v1x_kernel(const GemmArgs args) {
  constexpr int BK = 64, ROWB = BK * 2;
  constexpr int NT = WGN * WGM * 64;
  constexpr int WTN = TN / WGN, WTM = TM / WGM;
  constexpr int FN = WTN / 16, FM = WTM / 16;
  constexpr int IW = TN * 8 / NT, IX = TM * 8 / NT;
  static_assert(TN * 8 % NT == 0 && TM * 8 % NT == 0, "tile/threads mismatch");
  constexpr int BUF = (TN + TM) * ROWB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned long long t_entry = STAMP ? stamp() : 0;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn0 = (wave / WGM) * WTN;
  const int wm0 = (wave % WGM) * WTM;
  int n0, m0;
  const GemmProb& P = pick_tile<TN, TM>(args, n0, m0);
  const int K = P.K, M = P.M;

  const char* srcW[IW];
  const char* srcX[IX];
#pragma unroll
  for (int i = 0; i < IW; ++i) {
    const int q = tid + i * NT;
    const int row = q >> 3, c = (q & 7) ^ ((row >> 1) & 7);
    srcW[i] = (const char*)P.W + ((long long)(n0 + row) * K + c * 8) * 2;
  }
#pragma unroll
  for (int i = 0; i < IX; ++i) {
    const int q = tid + i * NT;
    const int row = q >> 3, c = (q & 7) ^ ((row >> 1) & 7);
    const int m = min(m0 + row, M - 1);
    srcX[i] = (const char*)P.A + (view_off(P.a, m) + c * 8) * 2;
  }
  const int wave_q0 = wave * 64;
  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * BUF;
    const long long koff = (long long)kt * ROWB;
#pragma unroll
    for (int i = 0; i < IW; ++i) glds16(srcW[i] + koff, base + (wave_q0 + i * NT) * 16);
#pragma unroll
    for (int i = 0; i < IX; ++i) glds16(srcX[i] + koff, base + TN * ROWB + (wave_q0 + i * NT) * 16);
  };
  int foff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int r = lane & 15;
    const int c = (4 * ks + (lane >> 4)) ^ ((r >> 1) & 7);
    foff[ks] = r * ROWB + c * 16;
  }
  f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = K / BK;
  const int spread_phase = (wave >= (WGN * WGM) / 2) ? 1 : 0;  // waves w and w + half share a SIMD
  // L2 prefetch: line q of a stage = row q of the W tile (q < TN) or row q - TN of the X tile
  const char* pfsrc = nullptr;
  char* pfdst = smem + 2 * BUF + wave * 512;
  if (PF) {
    const int q = tid % (TN + TM);
    if (q < TN) pfsrc = (const char*)P.W + (long long)(n0 + q) * K * 2;
    else pfsrc = (const char*)P.A + view_off(P.a, min(m0 + q - TN, M - 1)) * 2;
  }
  auto prefetch = [&](int kt) {
    __builtin_amdgcn_global_load_lds(MRA_GLB_PTR(pfsrc + (long long)kt * ROWB), MRA_LDS_PTR(pfdst), 4, 0, 0);
    __builtin_amdgcn_global_load_lds(MRA_GLB_PTR(pfsrc + (long long)kt * ROWB), MRA_LDS_PTR(pfdst), 4, 64, 0);
  };
  if (PF) {
    if (1 < nk) prefetch(1);
    if (2 < nk) prefetch(2);
  }
  stage(0, 0);
  unsigned long long tsum[4] = {0, 0, 0, 0}, tq[5];
  const unsigned long long t_loop0 = STAMP ? stamp() : 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (STAMP) {
      tq[0] = stamp();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      tq[1] = stamp();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      tq[2] = stamp();
    } else if (PF) {
      // the two youngest operations are the prefetch of tile kt + 2 (if one was issued): leave them in flight
      if (kt >= 1 && kt + 2 < nk) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    const bool more = kt + 1 < nk;
    if (!SPREAD && more) stage((kt + 1) & 1, kt + 1);
    if (STAMP) tq[3] = stamp();
    if (PF && kt + 3 < nk) prefetch(kt + 3);
    const char* wb = smem + (kt & 1) * BUF + wn0 * ROWB;
    const char* xb = smem + (kt & 1) * BUF + TN * ROWB + wm0 * ROWB;
    char* nbase = smem + ((kt + 1) & 1) * BUF;
    const long long nkoff = (long long)(kt + 1) * ROWB;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      typename Vec8<T>::type a[FN], b[FM];
#pragma unroll
      for (int i = 0; i < FN; ++i) a[i] = lds_read8<T>(wb + i * 16 * ROWB + foff[ks]);
#pragma unroll
      for (int j = 0; j < FM; ++j) b[j] = lds_read8<T>(xb + j * 16 * ROWB + foff[ks]);
#pragma unroll
      for (int i = 0; i < FN; ++i) {
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(a[i], b[j], acc[i][j]);
        if constexpr (SPREAD) {
          // group index 0 .. 2*FN-1; IW + IX loads are spread over the groups, phase-shifted per wave half
          constexpr int NG = 2 * FN, NL = IW + IX;
          static_assert(NG % NL == 0, "loads must divide the MFMA groups");
          constexpr int STEP = NG / NL;
          const int gi = ks * FN + i;
          if (more && (gi % STEP) == (STEP > 1 ? spread_phase : 0)) {
            const int l = gi / STEP;  // compile-time after unrolling
            if (l < IW) glds16(srcW[l] + nkoff, nbase + (wave_q0 + l * NT) * 16);
            else glds16(srcX[l - IW] + nkoff, nbase + TN * ROWB + (wave_q0 + (l - IW) * NT) * 16);
          }
        }
      }
    }
    if (STAMP) {
      tq[4] = stamp();
#pragma unroll
      for (int e = 0; e < 4; ++e) tsum[e] += tq[e + 1] - tq[e];
    }
  }
  const unsigned long long t_loop1 = STAMP ? stamp() : 0;
  if constexpr (EPI == EPI_OP || EPI == EPI_GELU_OP || EPI == EPI_KV) {
    __syncthreads();
    epilogue_lds16<T, TN, TM, FN, FM, NT, EPI>(P, acc, smem, n0, m0, wn0, wm0, tid);
  } else {
    epilogue<T, FN, FM, EPI>(P, acc, n0 + wn0, m0 + wm0, lane);
  }
  if (STAMP && args.dbg && lane == 0 && blockIdx.x < 4096) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned long long t_end = stamp();
    unsigned long long* d = args.dbg + ((size_t)blockIdx.x * (WGN * WGM) + wave) * 8;
    d[0] = tsum[0]; d[1] = tsum[1]; d[2] = tsum[2]; d[3] = tsum[3];
    d[4] = t_loop0 - t_entry; d[5] = t_loop1 - t_loop0; d[6] = t_end - t_loop1; d[7] = t_entry;
  }
}

// =================================================================================================
// ws2: warp-specialised 256x256, 4-slot LDS ring of 32-deep K slices, NO barrier in the K loop
// =================================================================================================
// With a barrier per K tile every compute wave restarts in lockstep: the two waves of a SIMD read
// their first fragments at the same moment and the matrix pipe idles ~900 of ~3000 cycles per tile
// ("ws without DMA" still stops at 1.25 PF).  Here loaders and compute waves hand slots over through
// monotonic LDS counters instead: full[s] (+1 by the slot's loader wave when its DMA has landed:
// vmcnt(0), then ds_add) and done[s] (+1 per compute wave after its last fragment read of the slot).
// A compute wave waits for full[s] >= use + 1 -- the poll for the next slot is issued early and
// normally already satisfied -- and never meets the other waves, so SIMD partners drift apart and
// cover each other's read bubbles; loader wave s refills slot s once done[s] >= 8 * use, so up to 3
// slots are in flight or landed ahead of the one being consumed.  Every spin is bounded (a hung grid would take the GPU down): on give-up the
// kernel finishes with wrong data and sets args.dbg[0] if a debug buffer is installed.
__device__ __forceinline__ bool spin_ge(volatile unsigned* p, unsigned target) {
  for (int i = 0; i < (1 << 16); ++i) {  // ~5 ms; a real wait is a few microseconds
    if (*p >= target) return true;
    __builtin_amdgcn_s_sleep(1);
  }
  return false;
}

template <typename T, int EPI>
__global__ void __launch_bounds__(768) gemm_ws2_kernel(const GemmArgs args) {
  constexpr int TN = 256, TM = 256, SK = 32, SROW = SK * 2, NS = 4;
  constexpr int WGM = 4, WTN = 128, WTM = 64, FN = 8, FM = 4;
  constexpr int SLOT = (TN + TM) * SROW;  // 32 KiB
  extern __shared__ __attribute__((aligned(16))) char smem[];
  volatile unsigned* full = reinterpret_cast<volatile unsigned*>(smem + NS * SLOT);
  volatile unsigned* done = full + NS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int n0, m0;
  const GemmProb& P = pick_tile<TN, TM>(args, n0, m0);
  const int K = P.K, M = P.M;
  const int nslots = K / SK;
  if (tid < 2 * NS) full[tid] = 0;
  __syncthreads();
  bool ok = true;

  if (wave >= 8) {
    // ------------------------------- loader waves -------------------------------
    // loader lw owns ring slot lw: it refills it (one 32 KiB slot = 32 LDS-DMA instructions of this
    // wave) as soon as all 8 compute waves are done with the previous occupant, and signals it the
    // moment the data has landed -- no loader ever waits on another slot's consumers.
    const int lw = wave - 8;
    // chunk q = lane + 64 i of an operand image (1024 chunks): row = (lane >> 2) + 16 i, physical chunk
    // lane & 3, and the swizzle term (-(row >> 2)) & 3 = (-(lane >> 4)) & 3 does not depend on i
    const int row0 = lane >> 2;
    const int c = (lane & 3) ^ ((-(lane >> 4)) & 3);
    const char* srcW = (const char*)P.W + ((long long)(n0 + row0) * K + c * 8) * 2;
    const long long strideW = (long long)16 * K * 2;
    const char* srcX[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int m = min(m0 + row0 + 16 * i, M - 1);
      srcX[i] = (const char*)P.A + (view_off(P.a, m) + c * 8) * 2;
    }
    for (int t = lw; t < nslots; t += NS) {
      const int use = t / NS;
      if (use > 0 && ok) ok = spin_ge(done + lw, 8u * use);  // after a give-up: run through, never wait again
      asm volatile("" ::: "memory");
      char* base = smem + lw * SLOT;
      const long long koff = (long long)t * SROW;
#pragma unroll
      for (int i = 0; i < 16; ++i) glds16(srcW + i * strideW + koff, base + i * 1024);
#pragma unroll
      for (int i = 0; i < 16; ++i) glds16(srcX[i] + koff, base + TN * SROW + i * 1024);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (lane == 0) atomicAdd(const_cast<unsigned*>(full) + lw, 1u);
    }
  } else {
    // --------------------------------- compute waves ---------------------------------
    const int wn0 = (wave / WGM) * WTN;
    const int wm0 = (wave % WGM) * WTM;
    const int foff = (lane & 15) * SROW + ((((lane >> 4)) ^ ((-((lane & 15) >> 2)) & 3)) << 4);
    f32x4 acc[FN][FM];
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned seen = full[0];
    for (int t = 0; t < nslots; ++t) {
      const int s = t & (NS - 1), use = t / NS;
      if (seen < (unsigned)(use + 1) && ok) ok = spin_ge(full + s, (unsigned)(use + 1));
      asm volatile("" ::: "memory");
      if (t + 1 < nslots) seen = full[(t + 1) & (NS - 1)];  // early poll for the next slot
      const char* wb = smem + s * SLOT + wn0 * SROW + foff;
      const char* xb = smem + s * SLOT + TN * SROW + wm0 * SROW + foff;
      typename Vec8<T>::type b[FM];
#pragma unroll
      for (int j = 0; j < FM; ++j) b[j] = lds_read8<T>(xb + j * 16 * SROW);
      typename Vec8<T>::type a_cur = lds_read8<T>(wb);
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        typename Vec8<T>::type a_nxt = a_cur;
        if (i + 1 < FN) a_nxt = lds_read8<T>(wb + (i + 1) * 16 * SROW);
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(a_cur, b[j], acc[i][j]);
        a_cur = a_nxt;
      }
      asm volatile("" ::: "memory");  // the slot's reads are all consumed by MFMAs issued above
      if (lane == 0) atomicAdd(const_cast<unsigned*>(done) + s, 1u);
    }
    if (!ok && args.dbg && lane == 0) args.dbg[0] = 1;
    __syncthreads();  // pairs with the loaders' barrier below: every slot read is over
    if constexpr (EPI == EPI_OP || EPI == EPI_GELU_OP || EPI == EPI_KV) {
      epilogue_lds16<T, TN, TM, FN, FM, 512, EPI>(P, acc, smem, n0, m0, wn0, wm0, tid);
    } else {
      epilogue<T, FN, FM, EPI>(P, acc, n0 + wn0, m0 + wm0, lane);
    }
    return;
  }
  if (!ok && args.dbg && lane == 0) args.dbg[0] = 1;
  __syncthreads();
  if constexpr (EPI == EPI_OP || EPI == EPI_GELU_OP || EPI == EPI_KV) __syncthreads();  // the one inside epilogue_lds16
}


// =================================================================================================
// 9 rot: two-buffer 256x256x64 loop with the second half of every K tile deferred past the barrier
// =================================================================================================
// Every wave reads the ks = 1 fragments of tile kt BEFORE barrier kt+1 and issues their 32 MFMAs AFTER
// it, interleaved with the 8 LDS-DMA instructions of tile kt+2 and in the shadow of the first fragment
// reads of tile kt+1: the barrier skew, the DMA issue and the read bubble all sit behind queued matrix
// work instead of in front of it.  8 waves (2 per SIMD, 224+ VGPRs), no loader waves.
template <typename T, int EPI>
__global__ void __launch_bounds__(512) gemm_rot_kernel(const GemmArgs args) {
  constexpr int TN = 256, TM = 256, BK = 64, ROWB = BK * 2, NT = 512;
  constexpr int WGM = 4, WTN = 128, WTM = 64, FN = 8, FM = 4;
  constexpr int BUF = (TN + TM) * ROWB;
  typedef typename Vec8<T>::type Frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn0 = (wave / WGM) * WTN;
  const int wm0 = (wave % WGM) * WTM;
  int n0, m0;
  const GemmProb& P = pick_tile<TN, TM>(args, n0, m0);
  const int K = P.K, M = P.M;
  const char* src[8];  // 0..3 W chunks, 4..7 X chunks
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int q = tid + (i & 3) * NT;
    const int row = q >> 3, c = (q & 7) ^ ((row >> 1) & 7);
    if (i < 4) src[i] = (const char*)P.W + ((long long)(n0 + row) * K + c * 8) * 2;
    else src[i] = (const char*)P.A + (view_off(P.a, min(m0 + row, M - 1)) + c * 8) * 2;
  }
  const int wave_q0 = wave * 64;
  auto dma1 = [&](int buf, int kt, int i) {
    glds16(src[i] + (long long)kt * ROWB, smem + buf * BUF + (i < 4 ? 0 : TN * ROWB) + (wave_q0 + (i & 3) * NT) * 16);
  };
  int foff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int r = lane & 15;
    foff[ks] = r * ROWB + (((4 * ks + (lane >> 4)) ^ ((r >> 1) & 7)) << 4);
  }
  f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  Frag fa[FN], fb[FM];  // the deferred half (ks = 1) of the previous tile

  auto read_half = [&](int buf, int ks, Frag (&a)[FN], Frag (&b)[FM]) {
    const char* wb = smem + buf * BUF + wn0 * ROWB + foff[ks];
    const char* xb = smem + buf * BUF + TN * ROWB + wm0 * ROWB + foff[ks];
#pragma unroll
    for (int j = 0; j < FM; ++j) b[j] = lds_read8<T>(xb + j * 16 * ROWB);
#pragma unroll
    for (int i = 0; i < FN; ++i) a[i] = lds_read8<T>(wb + i * 16 * ROWB);
  };
  // ks = 0 half of tile in `buf`, fragments just in time (keeps the register count under 256)
  auto mma_first_half = [&](int buf) {
    const char* wb = smem + buf * BUF + wn0 * ROWB + foff[0];
    const char* xb = smem + buf * BUF + TN * ROWB + wm0 * ROWB + foff[0];
    Frag b[FM];
#pragma unroll
    for (int j = 0; j < FM; ++j) b[j] = lds_read8<T>(xb + j * 16 * ROWB);
    Frag a_cur = lds_read8<T>(wb);
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      Frag a_nxt = a_cur;
      if (i + 1 < FN) a_nxt = lds_read8<T>(wb + (i + 1) * 16 * ROWB);
#pragma unroll
      for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(a_cur, b[j], acc[i][j]);
      a_cur = a_nxt;
    }
  };

  const int nk = K / BK;
#pragma unroll
  for (int i = 0; i < 8; ++i) dma1(0, 0, i);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (nk > 1) {
#pragma unroll
    for (int i = 0; i < 8; ++i) dma1(1, 1, i);
  }
  read_half(0, 1, fa, fb);
  mma_first_half(0);
  for (int kt = 1; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile kt landed; every fragment of tile kt-1 is in registers (fa/fb) or consumed
    const bool more = kt + 1 < nk;
    // deferred half of tile kt-1, one LDS-DMA of tile kt+1 between MFMA groups (its buffer is tile kt-1's)
#pragma unroll
    for (int i = 0; i < FN; ++i) {
#pragma unroll
      for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(fa[i], fb[j], acc[i][j]);
      if (more) dma1((kt + 1) & 1, kt + 1, i);
    }
    read_half(kt & 1, 1, fa, fb);
    mma_first_half(kt & 1);
  }
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(fa[i], fb[j], acc[i][j]);
  if constexpr (EPI == EPI_OP || EPI == EPI_GELU_OP || EPI == EPI_KV) {
    __syncthreads();
    epilogue_lds16<T, TN, TM, FN, FM, NT, EPI>(P, acc, smem, n0, m0, wn0, wm0, tid);
  } else {
    epilogue<T, FN, FM, EPI>(P, acc, n0 + wn0, m0 + wm0, lane);
  }
}

// =================================================================================================
// 10 w4: the same loop on FOUR waves of 128 x 128 (256 accumulator registers, one wave per SIMD)
// =================================================================================================
// 128 KB of fragment reads per 64-deep step instead of the 192 KB of eight 128 x 64 waves: LDS time 50 % instead of 75 % of MFMA time; the
// wave's own MFMA queue has to hide its fragment reads (nobody else is on the SIMD).  Structure of 9 rot:
// Every wave reads the ks = 1 fragments of tile kt BEFORE barrier kt+1 and issues their 64 MFMAs AFTER
// it, interleaved with the 8 LDS-DMA instructions of tile kt+2 and in the shadow of the first fragment
// reads of tile kt+1: the barrier skew, the DMA issue and the read bubble all sit behind queued matrix
// work instead of in front of it.  8 waves (2 per SIMD, 224+ VGPRs), no loader waves.
template <typename T, int EPI>
__global__ void __launch_bounds__(256) gemm_w4_kernel(const GemmArgs args) {
  constexpr int TN = 256, TM = 256, BK = 64, ROWB = BK * 2, NT = 256;
  constexpr int WGM = 2, WTN = 128, WTM = 128, FN = 8, FM = 8;
  constexpr int BUF = (TN + TM) * ROWB;
  typedef typename Vec8<T>::type Frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn0 = (wave / WGM) * WTN;
  const int wm0 = (wave % WGM) * WTM;
  int n0, m0;
  const GemmProb& P = pick_tile<TN, TM>(args, n0, m0);
  const int K = P.K, M = P.M;
  const char* src[16];  // 0..7 W chunks, 8..15 X chunks
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int q = tid + (i & 7) * NT;
    const int row = q >> 3, c = (q & 7) ^ ((row >> 1) & 7);
    if (i < 8) src[i] = (const char*)P.W + ((long long)(n0 + row) * K + c * 8) * 2;
    else src[i] = (const char*)P.A + (view_off(P.a, min(m0 + row, M - 1)) + c * 8) * 2;
  }
  const int wave_q0 = wave * 64;
  auto dma1 = [&](int buf, int kt, int i) {
    glds16(src[i] + (long long)kt * ROWB, smem + buf * BUF + (i < 8 ? 0 : TN * ROWB) + (wave_q0 + (i & 7) * NT) * 16);
  };
  int foff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int r = lane & 15;
    foff[ks] = r * ROWB + (((4 * ks + (lane >> 4)) ^ ((r >> 1) & 7)) << 4);
  }
  f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  Frag fa[FN], fb[FM];  // the deferred half (ks = 1) of the previous tile

  auto read_half = [&](int buf, int ks, Frag (&a)[FN], Frag (&b)[FM]) {
    const char* wb = smem + buf * BUF + wn0 * ROWB + foff[ks];
    const char* xb = smem + buf * BUF + TN * ROWB + wm0 * ROWB + foff[ks];
#pragma unroll
    for (int j = 0; j < FM; ++j) b[j] = lds_read8<T>(xb + j * 16 * ROWB);
#pragma unroll
    for (int i = 0; i < FN; ++i) a[i] = lds_read8<T>(wb + i * 16 * ROWB);
  };
  // ks = 0 half of tile in `buf`, fragments just in time (keeps the register count under 256)
  auto mma_first_half = [&](int buf) {
    const char* wb = smem + buf * BUF + wn0 * ROWB + foff[0];
    const char* xb = smem + buf * BUF + TN * ROWB + wm0 * ROWB + foff[0];
    Frag b[FM];
#pragma unroll
    for (int j = 0; j < FM; ++j) b[j] = lds_read8<T>(xb + j * 16 * ROWB);
    Frag a_cur = lds_read8<T>(wb);
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      Frag a_nxt = a_cur;
      if (i + 1 < FN) a_nxt = lds_read8<T>(wb + (i + 1) * 16 * ROWB);
#pragma unroll
      for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(a_cur, b[j], acc[i][j]);
      a_cur = a_nxt;
    }
  };

  const int nk = K / BK;
#pragma unroll
  for (int i = 0; i < 16; ++i) dma1(0, 0, i);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (nk > 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) dma1(1, 1, i);
  }
  read_half(0, 1, fa, fb);
  mma_first_half(0);
  for (int kt = 1; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile kt landed; every fragment of tile kt-1 is in registers (fa/fb) or consumed
    const bool more = kt + 1 < nk;
    // deferred half of tile kt-1, one LDS-DMA of tile kt+1 between MFMA groups (its buffer is tile kt-1's)
#pragma unroll
    for (int i = 0; i < FN; ++i) {
#pragma unroll
      for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(fa[i], fb[j], acc[i][j]);
      if (more) { dma1((kt + 1) & 1, kt + 1, 2 * i); dma1((kt + 1) & 1, kt + 1, 2 * i + 1); }
    }
    read_half(kt & 1, 1, fa, fb);
    mma_first_half(kt & 1);
  }
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(fa[i], fb[j], acc[i][j]);
  if constexpr (EPI == EPI_OP || EPI == EPI_GELU_OP || EPI == EPI_KV) {
    __syncthreads();
    epilogue_lds16<T, TN, TM, FN, FM, NT, EPI>(P, acc, smem, n0, m0, wn0, wm0, tid);
  } else {
    epilogue<T, FN, FM, EPI>(P, acc, n0 + wn0, m0 + wm0, lane);
  }
}

// =================================================================================================
// 11 w4p: four waves of 128 x 128, every fragment read issued one half-tile (64 MFMAs) ahead of its use
// =================================================================================================
// Two register sets of fragments (fa / fb, ga / gb: 128 VGPRs; the 256 accumulators live in AGPRs).  Per K tile, after ONE barrier:
//   phase A: the 64 MFMAs of (tile kt-1, ks 1) from fa / fb, and between their groups of eight the 16 LDS-DMA instructions of tile kt+1 and
//            the 16 fragment reads of (tile kt, ks 0) into ga / gb;
//   phase B: the 64 MFMAs of (tile kt, ks 0) from ga / gb, and between their groups the 16 fragment reads of (tile kt, ks 1) into fa / fb.
// With one wave per SIMD nobody else hides a wave's LDS latency: here every read has 1024 cycles of queued matrix work behind it.
template <typename T, int EPI>
__global__ void __launch_bounds__(256) gemm_w4p_kernel(const GemmArgs args) {
  constexpr int TN = 256, TM = 256, BK = 64, ROWB = BK * 2, NT = 256;
  constexpr int WGM = 2, WTN = 128, WTM = 128, FN = 8, FM = 8;
  constexpr int BUF = (TN + TM) * ROWB;
  typedef typename Vec8<T>::type Frag;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn0 = (wave / WGM) * WTN;
  const int wm0 = (wave % WGM) * WTM;
  int n0, m0;
  const GemmProb& P = pick_tile<TN, TM>(args, n0, m0);
  const int K = P.K, M = P.M;
  const char* src[16];  // 0..7 W chunks, 8..15 X chunks
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int q = tid + (i & 7) * NT;
    const int row = q >> 3, c = (q & 7) ^ ((row >> 1) & 7);
    if (i < 8) src[i] = (const char*)P.W + ((long long)(n0 + row) * K + c * 8) * 2;
    else src[i] = (const char*)P.A + (view_off(P.a, min(m0 + row, M - 1)) + c * 8) * 2;
  }
  const int wave_q0 = wave * 64;
  auto dma1 = [&](int buf, int kt, int i) {
    glds16(src[i] + (long long)kt * ROWB, smem + buf * BUF + (i < 8 ? 0 : TN * ROWB) + (wave_q0 + (i & 7) * NT) * 16);
  };
  int foff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int r = lane & 15;
    foff[ks] = r * ROWB + (((4 * ks + (lane >> 4)) ^ ((r >> 1) & 7)) << 4);
  }
  f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  Frag fa[FN], fb[FM], ga[FN], gb[FM];
  auto rd_a = [&](int buf, int ks, int i) { return lds_read8<T>(smem + buf * BUF + wn0 * ROWB + foff[ks] + i * 16 * ROWB); };
  auto rd_b = [&](int buf, int ks, int j) { return lds_read8<T>(smem + buf * BUF + TN * ROWB + wm0 * ROWB + foff[ks] + j * 16 * ROWB); };

  const int nk = K / BK;
#pragma unroll
  for (int i = 0; i < 16; ++i) dma1(0, 0, i);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (nk > 1) {
#pragma unroll
    for (int i = 0; i < 16; ++i) dma1(1, 1, i);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) { ga[i] = rd_a(0, 0, i); gb[i] = rd_b(0, 0, i); }
  // phase B of tile 0
#pragma unroll
  for (int i = 0; i < FN; ++i) {
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(ga[i], gb[j], acc[i][j]);
    fa[i] = rd_a(0, 1, i); fb[i] = rd_b(0, 1, i);
  }
  for (int kt = 1; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // tile kt landed; every fragment of tile kt-1 is in registers
    const int cur = kt & 1;
    const bool more = kt + 1 < nk;
    // phase A
#pragma unroll
    for (int i = 0; i < FN; ++i) {
#pragma unroll
      for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(fa[i], fb[j], acc[i][j]);
      if (more) { dma1(cur ^ 1, kt + 1, 2 * i); dma1(cur ^ 1, kt + 1, 2 * i + 1); }
      ga[i] = rd_a(cur, 0, i); gb[i] = rd_b(cur, 0, i);
    }
    // phase B
#pragma unroll
    for (int i = 0; i < FN; ++i) {
#pragma unroll
      for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(ga[i], gb[j], acc[i][j]);
      fa[i] = rd_a(cur, 1, i); fb[i] = rd_b(cur, 1, i);
    }
  }
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(fa[i], fb[j], acc[i][j]);
  if constexpr (EPI == EPI_OP || EPI == EPI_GELU_OP || EPI == EPI_KV) {
    __syncthreads();
    epilogue_lds16<T, TN, TM, FN, FM, NT, EPI>(P, acc, smem, n0, m0, wn0, wm0, tid);
  } else {
    epilogue<T, FN, FM, EPI>(P, acc, n0 + wn0, m0 + wm0, lane);
  }
}

// The 128 x 512 tail tile with the statistics epilogues: launch_gemm has no way to them (the mixed kernel is the one that runs a tail tile with
// statistics), but with them in the translation unit the compiler keeps the tile body they share with gemm_p8_mixed_kernel as it was when
// that kernel was measured -- this library is the measuring instrument (gemm_bench), so its code does not move with the dispatcher
template __global__ void gemm_p8_kernel<f16, EPI_RES_OP_STAT, true>(const GemmArgs);
template __global__ void gemm_p8_kernel<f16, EPI_RES_F32_STAT, true>(const GemmArgs);
template __global__ void gemm_p8_kernel<bf16, EPI_RES_OP_STAT, true>(const GemmArgs);
template __global__ void gemm_p8_kernel<bf16, EPI_RES_F32_STAT, true>(const GemmArgs);

using EpiW4 = Epis<EPI_OP, EPI_GELU_OP, EPI_KV>;
template <typename T>
int launch_w4p(const GemmArgs& a, int epi, hipStream_t stream) {
  constexpr size_t lds = 2 * (256 + 256) * 128;
  return with_epi(EpiW4{}, epi, [&](auto e) { return launch_k(gemm_w4p_kernel<T, e()>, a, 256, lds, stream); });
}
template <typename T>
int launch_w4(const GemmArgs& a, int epi, hipStream_t stream) {
  constexpr size_t lds = 2 * (256 + 256) * 128;
  return with_epi(EpiW4{}, epi, [&](auto e) { return launch_k(gemm_w4_kernel<T, e()>, a, 256, lds, stream); });
}
template <typename T>
int launch_rot(const GemmArgs& a, int epi, hipStream_t stream) {
  constexpr size_t lds = 2 * (256 + 256) * 128;
  return with_epi(EpiDirect{}, epi, [&](auto e) { return launch_k(gemm_rot_kernel<T, e()>, a, 512, lds, stream); });
}
template <typename T, int TN, int TM, int WGN, int WGM, int NS, int SPI>
int launch_ring(const GemmArgs& a, int epi, hipStream_t stream) {
  constexpr size_t lds = (size_t)NS * (TN + TM) * 64;
  return with_epi(EpiDirect{}, epi, [&](auto e) { return launch_k(gemm_ring_kernel<T, TN, TM, WGN, WGM, NS, SPI, e()>, a, WGN * WGM * 64, lds, stream); });
}
template <typename T, int TN, int TM, int WGN, int WGM, bool PF, bool SPREAD>
int launch_v1x(const GemmArgs& a, int epi, hipStream_t stream) {
  constexpr size_t lds = 2 * (TN + TM) * 128 + (PF ? WGN * WGM * 512 : 0);
  return with_epi(EpiDirect{}, epi, [&](auto e) { return launch_k(gemm_v1x_kernel<T, TN, TM, WGN, WGM, e(), PF, SPREAD>, a, WGN * WGM * 64, lds, stream); });
}
template <typename T>
int launch_ws2(const GemmArgs& a, int epi, hipStream_t stream) {
  constexpr size_t lds = 4 * (256 + 256) * 64 + 64;
  return with_epi(EpiDirect{}, epi, [&](auto e) { return launch_k(gemm_ws2_kernel<T, e()>, a, 768, lds, stream); });
}
template <typename T, int TN, int TM, int WGN, int WGM>
int launch_k128(const GemmArgs& a, int epi, hipStream_t stream) {
  constexpr size_t lds = 2 * (TN + TM) * 256;
  return with_epi(EpiDirect{}, epi, [&](auto e) { return launch_k(gemm_k128_kernel<T, TN, TM, WGN, WGM, e()>, a, WGN * WGM * 64, lds, stream); });
}

// `variant` as an experiment's main loop for `tile` (GT_64 / GT_128 / GT_256): true and *rc = the launch's result; false when the variant
// has none for this tile and epilogue (the caller then takes the shipped path)
template <typename T>
bool launch_experiment(const GemmArgs& a, int tile, int epi, int variant, hipStream_t stream, int* rc) {
  switch (variant) {
    case 0:
      *rc = tile == GT_256 ? launch_ring<T, 256, 256, 2, 4, 5, 2>(a, epi, stream) : tile == GT_128 ? launch_ring<T, 128, 128, 2, 2, 6, 2>(a, epi, stream) : launch_ring<T, 64, 64, 2, 2, 8, 2>(a, epi, stream);
      return true;
    case 2:
      *rc = tile == GT_256 ? launch_v1x<T, 256, 256, 2, 4, true, false>(a, epi, stream) : tile == GT_128 ? launch_v1x<T, 128, 128, 2, 2, true, false>(a, epi, stream) : launch_v1x<T, 64, 64, 2, 2, true, false>(a, epi, stream);
      return true;
    case 3:
      *rc = tile == GT_256 ? launch_v1x<T, 256, 256, 2, 4, false, true>(a, epi, stream) : tile == GT_128 ? launch_v1x<T, 128, 128, 2, 2, false, true>(a, epi, stream) : launch_v1x<T, 64, 64, 2, 2, false, true>(a, epi, stream);
      return true;
    case 4:
      if (tile != GT_256 || epi != EPI_KV) return false;
      *rc = launch_k(gemm_v1x_kernel<T, 256, 256, 2, 4, EPI_KV, false, false, true>, a, 512, 2 * 512 * 128, stream);
      return true;
    case 6:
      if (tile != GT_256 || epi != EPI_KV) return false;
      *rc = launch_k(gemm_ws_kernel<T, EPI_KV, true>, a, 768, 2 * 512 * 128, stream);
      return true;
    case 7:
    case 9:
    case 10:
    case 11:
      if (tile != GT_256) return false;
      *rc = variant == 7 ? launch_ws2<T>(a, epi, stream) : variant == 9 ? launch_rot<T>(a, epi, stream) : variant == 10 ? launch_w4<T>(a, epi, stream) : launch_w4p<T>(a, epi, stream);
      return true;
    case 8: {
      bool k128 = true;
      for (int g = 0; g < a.ngroups; ++g) k128 = k128 && a.p[g].K % 128 == 0;
      if (tile == GT_256 || !k128) return false;
      *rc = tile == GT_128 ? launch_k128<T, 128, 128, 2, 2>(a, epi, stream) : launch_k128<T, 64, 64, 2, 2>(a, epi, stream);
      return true;
    }
  }
  return false;
}
