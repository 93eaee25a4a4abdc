// Query-KV attention core for the Q-Former: softmax(Q K^T / 8 + mask) V with 64-wide heads.
//
// Used twice per layer on the path the reference drives at models/xinstructblip.py:286-293:
//   * self-attention over the S = 32 + L tokens of every item (additive text-padding mask,
//     LAVIS form (1 - m) * -10000), units = item x head x 32-row query block;
//   * cross-attention of the 32 learned queries onto the Kv encoder tokens of the item
//     (K/V projected once for all cross layers into a head-major cache, [Kv][64] per head).
//
// One wave owns one 32-query block.  KV tiles of 32 tokens are staged by LDS-DMA into a
// wave-private, double-buffered LDS ring (no workgroup barrier in the loop):
//   S^T[tok][q] = K_tile * Q^T            4 x v_mfma_f32_32x32x16 (K rows from LDS, Q in registers)
//   online softmax per query = per lane column (stats live in the lane, one lane<->lane+32 swap)
//   O^T[d][q] += V^T * P^T                4 x v_mfma_f32_32x32x16; P^T is the S^T accumulator
//                                         itself (rows are the contraction index), V^T comes
//                                         from ds_read_b64_tr_b16 transposed reads of [tok][d].
// LDS rows are 128 B: K chunks are XOR-swizzled with (tok >> 1) & 7 for conflict-free
// ds_read_b128, V chunks with ((tok >> 1) & 1) << 2 for conflict-free transposed reads; the
// swizzle is applied to the DMA source address (LDS-DMA writes linearly).
// Long KV (cross attention): the 4 waves of a workgroup take interleaved tiles of one unit and
// merge through LDS; optionally the KV range is also split over workgroups (partials merged by
// attn_combine_kernel) so that 384 (item, head) units still fill 256 CUs.
// Several prompts per clip (AttnArgs::kv_share > 1): attn_kernel takes the K/V of item n / kv_share; attn_shared_kernel below is the
// core built for that case, one workgroup-shared K/V ring under the query blocks of 4 prompts.
#include <atomic>
#include <type_traits>

#include "kernels.h"
#include "mra_common.h"

namespace mra {

namespace {

typedef int i32x4v __attribute__((ext_vector_type(4)));

constexpr int KVT = 32;                 // tokens per tile
constexpr int TILE_B = KVT * 128;       // bytes per K (or V) tile
constexpr int WAVE_LDS = 4 * TILE_B;    // 2 buffers x (K + V)
constexpr int OPAD = 68;                // padded row of the f32 O scratch
constexpr float LOG2E = 1.4426950408889634f;
constexpr int PART_STRIDE = 32 * 64 + 64;  // floats per partial: O[32][64], m[32], l[32]
// shared-stream core: a stage is SH_TPS tiles of K and V, the ring holds SH_STAGES stages (one barrier per stage)
constexpr int SH_TPS = 2;
constexpr int SH_STAGES = 3;
constexpr int SH_STAGE_B = SH_TPS * 2 * TILE_B;        // [tile][K tile | V tile]
constexpr int SH_PARK_B = (32 * OPAD + 64) * 4;        // one wave's O scratch + m + l
constexpr int SH_LDS = SH_STAGES * SH_STAGE_B > 4 * SH_PARK_B ? SH_STAGES * SH_STAGE_B : 4 * SH_PARK_B;

// One KV tile of 32 tokens under one wave's 32 queries: S^T = K Q^T, the online softmax in log2 units, O^T += V^T P^T.  kb: the K tile in
// LDS (128-byte rows, chunks XOR (tok >> 1) & 7), vtile: the LDS address of the V tile (chunks XOR ((tok >> 1) & 1) << 2), koff / vlane: the
// fragment read offsets of attn_kernel, qf: the Q fragments, wm: the additive mask of the tile's 32 tokens in log2 units (MASKED; -inf past
// kv_len).  Shared by attn_kernel and qkv_attn_kernel: the same instructions on the same operands, so the same bits.
template <typename T, bool MASKED>
__device__ __forceinline__ void attn_tile_step(const char* kb, unsigned vtile, const int (&koff)[4], const unsigned (&vlane)[2],
                                               const typename Vec8<T>::type (&qf)[4], const float* wm, int tok0, int kv_len, float sl2, int h4,
                                               float& m_run, float& l_run, f32x16 (&ot)[2]) {
  // S^T = K * Q^T
  f32x16 st;
#pragma unroll
  for (int i = 0; i < 16; ++i) st[i] = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) st = mfma32<T>(lds_read8<T>(kb + koff[s]), qf[s], st);

  // scores in log2 units, tail / padding mask
  float mx = -INFINITY;
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    f32x4 madd;
    if (MASKED) {
      madd = *reinterpret_cast<const f32x4*>(wm + 8 * g4 + h4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 4 * g4 + e;
      float y = st[i] * sl2;
      if (MASKED) {
        y += madd[e];
      } else {
        if (tok0 + 8 * g4 + h4 + e >= kv_len) y = -INFINITY;
      }
      st[i] = y;
      mx = fmaxf(mx, y);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float m_new = fmaxf(m_run, mx);
  const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
  m_run = m_new;
  float psum = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float p = __builtin_amdgcn_exp2f(st[i] - m_new);
    st[i] = p;
    psum += p;
  }
  l_run = l_run * alpha + psum;
#pragma unroll
  for (int i = 0; i < 16; ++i) { ot[0][i] *= alpha; ot[1][i] *= alpha; }

  // P^T fragments (B operand): k-step s uses accumulator registers 8 s .. 8 s + 7
  typename Vec8<T>::type pf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) pf[s][j] = from_f32<T>(st[8 * s + j]);

  // O^T += V^T * P^T.  The transposed reads go through inline asm: as compiler-visible LDS
  // loads hipcc orders them behind every pending LDS-DMA (s_waitcnt vmcnt(0)), which would
  // drain the prefetch of the next tile.  Loads and their wait sit in one statement.
  {
    const unsigned vaddr0 = vtile + vlane[0];
    const unsigned vaddr1 = vtile + vlane[1];
    i16x4 r00, r01, r02, r03, r10, r11, r12, r13;
    asm volatile(
        "ds_read_b64_tr_b16 %0, %8\n\t"
        "ds_read_b64_tr_b16 %1, %8 offset:1024\n\t"
        "ds_read_b64_tr_b16 %2, %8 offset:2048\n\t"
        "ds_read_b64_tr_b16 %3, %8 offset:3072\n\t"
        "ds_read_b64_tr_b16 %4, %9\n\t"
        "ds_read_b64_tr_b16 %5, %9 offset:1024\n\t"
        "ds_read_b64_tr_b16 %6, %9 offset:2048\n\t"
        "ds_read_b64_tr_b16 %7, %9 offset:3072\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(r00), "=&v"(r01), "=&v"(r02), "=&v"(r03), "=&v"(r10), "=&v"(r11), "=&v"(r12), "=&v"(r13)
        : "v"(vaddr0), "v"(vaddr1)
        : "memory");
    auto cat = [](i16x4 lo, i16x4 hi) {
      i16x8 v8;
      v8[0] = lo[0]; v8[1] = lo[1]; v8[2] = lo[2]; v8[3] = lo[3];
      v8[4] = hi[0]; v8[5] = hi[1]; v8[6] = hi[2]; v8[7] = hi[3];
      return __builtin_bit_cast(typename Vec8<T>::type, v8);
    };
    ot[0] = mfma32<T>(cat(r00, r01), pf[0], ot[0]);
    ot[0] = mfma32<T>(cat(r02, r03), pf[1], ot[0]);
    ot[1] = mfma32<T>(cat(r10, r11), pf[0], ot[1]);
    ot[1] = mfma32<T>(cat(r12, r13), pf[1], ot[1]);
  }
}

template <typename T, bool MASKED, int SPLITW>
__global__ void __launch_bounds__(256) attn_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qblocks = (a.q_rows + 31) >> 5;
  const int nunits = a.items * a.heads * qblocks;
  const int ntiles_all = (a.kv_len + KVT - 1) / KVT;

  // ---- which unit / which tile range ----
  int unit, gs;
  if (SPLITW == 1) {
    unit = blockIdx.x * 4 + wave;
    gs = 0;
  } else {
    unit = blockIdx.x / a.nsplit;
    gs = blockIdx.x - unit * a.nsplit;
  }
  const bool active = unit < nunits;
  if (!active) unit = nunits - 1;
  const int qb = unit % qblocks;
  const int head = (unit / qblocks) % a.heads;
  const int item = unit / (qblocks * a.heads);
  const int q0 = qb * 32;

  const int tps = (ntiles_all + a.nsplit - 1) / a.nsplit;  // tiles per grid split
  const int tb = gs * tps;
  const int te = min(tb + tps, ntiles_all);
  const int tstep = SPLITW;
  const int tfirst = tb + (SPLITW == 1 ? 0 : wave);

  char* wl = smem + wave * WAVE_LDS;  // this wave's ring: [buf][K tile | V tile]
  const int mask_pad = ntiles_all * KVT;
  float* wmask = reinterpret_cast<float*>(smem + 4 * WAVE_LDS) + wave * mask_pad;

  const int kv_item = item / a.kv_share;   // several prompts of one clip read one K/V stream (kv_share 1: every item its own)
  const T* Kb = (const T*)a.K + (long long)kv_item * a.k_item_stride + (long long)head * a.k_head_stride;
  const T* Vb = (const T*)a.V + (long long)kv_item * a.v_item_stride + (long long)head * a.v_head_stride;

  // ---- additive mask in log2 units (self attention only) ----
  if (MASKED) {
    for (int i = lane; i < mask_pad; i += 64) {
      float v = -INFINITY;
      if (i < a.kv_len) {
        const long long mv = a.mask ? a.mask[(long long)item * a.mask_ld + i] : 1;
        v = (1.0f - (float)mv) * (-10000.0f * LOG2E);
      }
      wmask[i] = v;
    }
  }

  // ---- Q fragments: B operand, lane (col q = lane & 31, half h) holds Q[q][16 s + 8 h + j] ----
  typename Vec8<T>::type qf[4];
  {
    const int qr = min(q0 + (lane & 31), a.q_rows - 1);
    const T* qp = (const T*)a.Q + (long long)item * a.q_item_stride + (long long)qr * a.q_ld + head * 64 + 8 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const typename Vec8<T>::type*>(qp + 16 * s);
  }

  // ---- per-lane LDS-DMA sources (row = 8 i + (lane >> 3), physical chunk = lane & 7) ----
  const int srow = lane >> 3, sc = lane & 7;
  auto issue = [&](int buf, int t) {
    char* kb = wl + buf * 2 * TILE_B;
    char* vb = kb + TILE_B;
    const int tok0 = t * KVT;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 8 * i + srow;
      const int tok = min(tok0 + row, a.kv_len - 1);
      const int kc = sc ^ ((row >> 1) & 7);
      const int vc = sc ^ (((row >> 1) & 1) << 2);
      glds16((const char*)(Kb + (long long)tok * a.k_ld) + kc * 16, kb + i * 1024);
      glds16((const char*)(Vb + (long long)tok * a.v_ld) + vc * 16, vb + i * 1024);
    }
  };

  // ---- fragment read addresses ----
  // K (A operand): lane (row tok = lane & 31, half h), k-step s: chunk 2 s + h
  int koff[4];
  {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) koff[s] = r * 128 + (((2 * s + h) ^ ((r >> 1) & 7)) << 4);
  }
  // V^T (A operand, rows d): 16-lane group g, lane-in-group i = 4 q4 + p reads 8 bytes of token row
  // T0 + q4 at d = 32 mt + 16 (g & 1) + 4 p; T0 = 16 s + 4 h (+ 8 for elements 4..7).  The V
  // swizzle bit ((row >> 1) & 1) equals (q4 >> 1) & 1 for every (s, e), so each d-half mt needs one
  // per-lane base and the (s, e) step is an immediate: 2048 s + 1024 e.
  unsigned vlane[2];
  {
    const int g = lane >> 4, i = lane & 15, q4 = i >> 2, p = i & 3, h = lane >> 5;
    const int row = 4 * h + q4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int c = 4 * mt + 2 * (g & 1) + (p >> 1);
      const int pc = c ^ (((q4 >> 1) & 1) << 2);
      vlane[mt] = row * 128 + pc * 16 + (p & 1) * 8;
    }
  }
  const unsigned wl_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)wl;

  const float sl2 = a.scale * LOG2E;
  float m_run = -1e30f, l_run = 0.f;
  f32x16 ot[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { ot[0][i] = 0.f; ot[1][i] = 0.f; }

  const int h4 = 4 * (lane >> 5);
  int buf = 0;
  if (tfirst < te) issue(0, tfirst);
  for (int t = tfirst; t < te; t += tstep) {
    const bool more = t + tstep < te;
    if (more) {
      issue(buf ^ 1, t + tstep);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const char* kb = wl + buf * 2 * TILE_B;
    attn_tile_step<T, MASKED>(kb, wl_lds + buf * 2 * TILE_B + TILE_B, koff, vlane, qf, MASKED ? wmask + t * KVT : nullptr, t * KVT, a.kv_len, sl2, h4,
                              m_run, l_run, ot);
    buf ^= 1;
  }

  // ---- merge ----
  // every wave parks (O unnormalised, m, l) in its own LDS region (the ring is idle now)
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  float* ow = reinterpret_cast<float*>(wl);
  float* mw = ow + 32 * OPAD;
  float* lw = mw + 32;
  {
    const int q = lane & 31;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        f32x4 v = {ot[mt][4 * g4], ot[mt][4 * g4 + 1], ot[mt][4 * g4 + 2], ot[mt][4 * g4 + 3]};
        *reinterpret_cast<f32x4*>(ow + q * OPAD + 32 * mt + 8 * g4 + h4) = v;
      }
    if (lane < 32) { mw[q] = m_run; lw[q] = l_tot; }
  }
  __syncthreads();

  constexpr int NW = SPLITW;                  // waves merged into one result
  const int tl = SPLITW == 1 ? lane : tid;    // thread index inside the merging group
  constexpr int NTHR = SPLITW == 1 ? 64 : 256;
  const char* gbase = SPLITW == 1 ? wl : smem;
  for (int idx = tl; idx < 256; idx += NTHR) {
    const int q = idx >> 3, dc = idx & 7;
    float M = -1e30f;
#pragma unroll
    for (int w = 0; w < NW; ++w) M = fmaxf(M, reinterpret_cast<const float*>(gbase + w * WAVE_LDS)[32 * OPAD + q]);
    float L = 0.f;
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float* rw = reinterpret_cast<const float*>(gbase + w * WAVE_LDS);
      const float wgt = __builtin_amdgcn_exp2f(rw[32 * OPAD + q] - M);
      L += wgt * rw[32 * OPAD + 32 + q];
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(rw + q * OPAD + 8 * dc);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(rw + q * OPAD + 8 * dc + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[e] += wgt * x0[e]; o[4 + e] += wgt * x1[e]; }
    }
    if (!active) continue;
    if (a.lse && a.nsplit == 1 && dc == 0 && q0 + q < a.q_rows)
      a.lse[((long long)item * a.heads + head) * a.q_rows + q0 + q] = M + __builtin_amdgcn_logf(L);  // v_log_f32 = log2
    if (a.nsplit > 1) {
      float* pp = a.part + ((long long)unit * a.nsplit + gs) * PART_STRIDE;
      *reinterpret_cast<f32x4*>(pp + q * 64 + 8 * dc) = f32x4{o[0], o[1], o[2], o[3]};
      *reinterpret_cast<f32x4*>(pp + q * 64 + 8 * dc + 4) = f32x4{o[4], o[5], o[6], o[7]};
      if (dc == 0) { pp[32 * 64 + q] = M; pp[32 * 64 + 32 + q] = L; }
    } else if (q0 + q < a.q_rows) {
      const float inv = 1.0f / L;
      typename Vec8<T>::type r;
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = from_f32<T>(o[e] * inv);
      T* op = (T*)a.O + (long long)item * a.o_item_stride + (long long)(q0 + q) * a.o_ld + head * 64 + 8 * dc;
      *reinterpret_cast<typename Vec8<T>::type*>(op) = r;
    }
  }
}

// merges the grid-split partials of one unit: 256 threads, thread (q = tid >> 3, dc = tid & 7)
template <typename T>
__global__ void __launch_bounds__(256) attn_combine_kernel(const AttnArgs a) {
  const int unit = blockIdx.x;
  const int qblocks = (a.q_rows + 31) >> 5;
  const int qb = unit % qblocks;
  const int head = (unit / qblocks) % a.heads;
  const int item = unit / (qblocks * a.heads);
  const int q = threadIdx.x >> 3, dc = threadIdx.x & 7;
  const float* pp = a.part + (long long)unit * a.nsplit * PART_STRIDE;
  float M = -1e30f;
  for (int s = 0; s < a.nsplit; ++s) M = fmaxf(M, pp[s * PART_STRIDE + 32 * 64 + q]);
  float L = 0.f;
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < a.nsplit; ++s) {
    const float* ps = pp + s * PART_STRIDE;
    const float wgt = __builtin_amdgcn_exp2f(ps[32 * 64 + q] - M);
    L += wgt * ps[32 * 64 + 32 + q];
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(ps + q * 64 + 8 * dc);
    const f32x4 x1 = *reinterpret_cast<const f32x4*>(ps + q * 64 + 8 * dc + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] += wgt * x0[e]; o[4 + e] += wgt * x1[e]; }
  }
  const int q0 = qb * 32;
  if (q0 + q >= a.q_rows) return;
  if (a.lse && dc == 0) a.lse[((long long)item * a.heads + head) * a.q_rows + q0 + q] = M + __builtin_amdgcn_logf(L);
  const float inv = 1.0f / L;
  typename Vec8<T>::type r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = from_f32<T>(o[e] * inv);
  T* op = (T*)a.O + (long long)item * a.o_item_stride + (long long)(q0 + q) * a.o_ld + head * 64 + 8 * dc;
  *reinterpret_cast<typename Vec8<T>::type*>(op) = r;
}

std::atomic<long long>& attn_launch_counter(bool masked);

template <typename T>
int launch_t(const AttnArgs& a, hipStream_t stream) {
  const int qblocks = (a.q_rows + 31) >> 5;
  const int nunits = a.items * a.heads * qblocks;
  const int ntiles = (a.kv_len + KVT - 1) / KVT;
  const bool masked = a.mask != nullptr;
  // short KV: one wave per unit, 4 units per workgroup; long KV: 4 waves share a unit
  const bool shared = ntiles >= 8 && !masked;
  size_t lds = 4 * WAVE_LDS + (masked ? (size_t)4 * ntiles * KVT * sizeof(float) : 0);
  if (lds > 160 * 1024) return -1;
  void (*kfn)(const AttnArgs);
  dim3 grid;
  if (shared) {
    kfn = attn_kernel<T, false, 4>;
    grid = dim3(nunits * a.nsplit);
  } else {
    if (a.nsplit != 1) return -1;
    kfn = masked ? attn_kernel<T, true, 1> : attn_kernel<T, false, 1>;
    grid = dim3((nunits + 3) / 4);
  }
  if (lds > 64 * 1024) {  // (self-attention with very long prompts only; a plain attribute call, not a stream op)
    if (hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return -3;
  }
  hipLaunchKernelGGL(kfn, grid, dim3(256), lds, stream, a);
  if (shared && a.nsplit > 1) {
    hipLaunchKernelGGL(attn_combine_kernel<T>, dim3(nunits), dim3(256), 0, stream, a);
  }
  if (hipGetLastError() != hipSuccess) return -4;
  if (!shared) attn_launch_counter(masked).fetch_add(1, std::memory_order_relaxed);
  return 0;
}

// =================================================================================================
// Fused Q|K|V projection + masked self-attention: steps 1 + 2 of a layer in ONE launch (mra_qformer_set_option "self_fuse")
// =================================================================================================
// A workgroup owns one head of G = 2 consecutive items (S <= 64 tokens each): 8 waves, the whole 160 KB of LDS, one workgroup per CU.
//   phase 1  [Q_h | K_h | V_h] of both items = X W^T for the head's 192 rows of wqkv (rows h * 64 .. + 63 of each of its three H-row
//            blocks) x 128 activation rows (item slot g = rows 64 g .. 64 g + 63, tokens past S and the item past N clamped: computed,
//            finite, never stored).  This is gemm_ring_kernel's loop on its 192 x 128 tile: 64-deep K tiles through a ring of 4 LDS
//            slots staged 2 ahead by LDS-DMA behind a counted vmcnt (one tile, 5 x 1 KiB pieces per wave, stays in flight across the
//            barrier), two groups of 4 waves on alternating K tiles -- one reads its tile's fragments while its SIMD partners multiply.
//            An output element is therefore the ring kernel's: the 16 x 16 x 32 MFMA chain of the even K tiles + the chain of the odd
//            ones + bias, rounded to the operand dtype -- the bits qkv16 holds after the chain's QKV launch on any ring tile.
//   hand-over  the groups exchange halves of their partial sums through the dead ring (as the ring kernel's epilogue), finish their half
//            and write it BEHIND the exchange area as the tiles the attention core reads: per item slot Q, K, V as [64 tokens][128 B],
//            Q and K chunks XOR (tok >> 1) & 7 (ds_read_b128 fragments), V chunks XOR ((tok >> 1) & 1) << 2 (transposed reads).
//   phase 2  waves 0 .. G * qblocks - 1 each own one (item slot, 32-query block): attn_kernel<T, true, 1>'s unit on attn_tile_step, the
//            tiles read where phase 1 left them, the mask row and the O scratch in the wave's own 16 KB of the dead exchange area; no
//            workgroup barrier after the hand-over.  ctx rows go where attn_kernel puts them, with its merge arithmetic (one partial).
struct QkvAttnArgs {
  const void* X;           // [N * S][H]
  const void* W;           // wqkv [3 H][H]
  const float* bias;       // [3 H] or nullptr
  const long long* mask;   // [N][S] or nullptr (all ones)
  void* O;                 // ctx [N * S][H]
  int N, S, H, heads;
  float scale;
};

template <typename T>
__global__ void __launch_bounds__(512) qkv_attn_kernel(const QkvAttnArgs a) {
  constexpr int BK = 64, ROWB = BK * 2, G = 2;
  constexpr int TN = 192, TM = 64 * G, WGN = 2, WGM = 2, STAGES = 4;
  constexpr int NWC = WGN * WGM, NW = 2 * NWC;
  constexpr int WTN = TN / WGN, WTM = TM / WGM, FN = WTN / 16, FM = WTM / 16;
  constexpr int ROWS = TN + TM, NPIECE = ROWS / 8, PPW = NPIECE / NW;
  constexpr int BUF = ROWS * ROWB;
  constexpr int RED_BYTES = NWC * FN * FM * 1024;
  constexpr int HEAD_B = 64 * ROWB, SLOT_B = 3 * HEAD_B;      // one of Q / K / V of an item slot; the slot's three
  constexpr int PRIV_B = 16384, PRIV_MASK = 32 * OPAD * 4 + 256;   // phase 2, per wave: O scratch + m + l, then the mask row
  static_assert(NPIECE == PPW * NW && (STAGES - 3) * PPW <= 63, "every wave stages PPW whole pieces per K tile; vmcnt holds 6 bits");
  static_assert(RED_BYTES + G * SLOT_B <= STAGES * BUF && (FN * FM) % 2 == 0, "exchange area + Q/K/V tiles reuse the ring");
  static_assert(4 * PRIV_B <= RED_BYTES && PRIV_MASK + 64 * 4 <= PRIV_B && WTM == 64, "phase 2 scratch lies in the exchange area");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using V8 = typename Vec8<T>::type;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int group = wave / NWC, gw = wave - group * NWC;
  const int wn0 = (gw / WGM) * WTN;
  const int wm0 = (gw % WGM) * WTM;
  const int head = blockIdx.x % a.heads, item0 = (blockIdx.x / a.heads) * G;
  const int S = a.S, H = a.H, N = a.N;
  const int nk = H / BK;

  // ---- phase 1 ----
  // this wave's pieces of every K tile: p = wave + i * NW; piece p = LDS rows 8 p .. 8 p + 7 (rows [0, TN) weights, then activations)
  const char* src[PPW];
#pragma unroll
  for (int i = 0; i < PPW; ++i) {
    const int p = wave + i * NW;
    const int row = p * 8 + (lane >> 3), c = (lane & 7) ^ ((row >> 1) & 7);
    if (row < TN) {   // wave-uniform
      const long long wr = (long long)(row >> 6) * H + head * 64 + (row & 63);
      src[i] = (const char*)a.W + (wr * H + c * 8) * 2;
    } else {
      const int m = row - TN;
      const int item = min(item0 + (m >> 6), N - 1), tok = min(m & 63, S - 1);
      src[i] = (const char*)a.X + (((long long)item * S + tok) * H + c * 8) * 2;
    }
  }
  auto stage = [&](int slot, int kt) {
    char* base = smem + slot * BUF + wave * 1024;
    const long long koff = (long long)kt * ROWB;
#pragma unroll
    for (int i = 0; i < PPW; ++i) glds16(src[i] + koff, base + i * (NW * 1024));
  };
#pragma unroll
  for (int t = 0; t < STAGES - 2; ++t)
    if (t < nk) stage(t, t);
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

  {
    V8 fa[2][FN], fb[2][FM];
    int rslot = 0, fslot = STAGES - 2;   // slots of tile kt and of tile kt + STAGES - 2
    // one interval of the ring kernel: the barrier that publishes tile kt, then this group's role (compile-time at each call site)
    auto interval = [&](auto GRP, auto PAR, int kt) {
      constexpr int g = decltype(GRP)::value, par = decltype(PAR)::value;
      // tile kt must have landed; tile kt + 1 (issued in the interval since) may stay in flight
      if (kt < nk) {
        if (kt + STAGES - 3 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((STAGES - 3) * PPW) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if constexpr (par == g) {
        if (kt < nk) {   // this group's turn: the fragments of tile kt into registers
          const char* wb = smem + rslot * BUF + wn0 * ROWB;
          const char* xb = smem + rslot * BUF + TN * ROWB + wm0 * ROWB;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int i = 0; i < FN; ++i) fa[ks][i] = lds_read8<T>(wb + i * 16 * ROWB + foff[ks]);
#pragma unroll
            for (int j = 0; j < FM; ++j) fb[ks][j] = lds_read8<T>(xb + j * 16 * ROWB + foff[ks]);
          }
        }
      } else {
        if (kt >= 1) {   // the MFMAs of tile kt - 1 (read in the previous interval)
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < FN; ++i)
#pragma unroll
              for (int j = 0; j < FM; ++j) acc[i][j] = mfma16<T>(fa[ks][i], fb[ks][j], acc[i][j]);
          __builtin_amdgcn_s_setprio(0);
        }
      }
      if (kt + STAGES - 2 < nk) stage(fslot, kt + STAGES - 2);   // the slot's last readers passed this barrier
      rslot = rslot + 1 == STAGES ? 0 : rslot + 1;
      fslot = fslot + 1 == STAGES ? 0 : fslot + 1;
    };
    auto run = [&](auto GRP) {
#pragma clang loop unroll(disable)
      for (int kt = 0; kt <= nk; kt += 2) {
        interval(GRP, std::integral_constant<int, 0>{}, kt);
        if (kt + 1 <= nk) interval(GRP, std::integral_constant<int, 1>{}, kt + 1);
      }
    };
    if (group == 0) run(std::integral_constant<int, 0>{}); else run(std::integral_constant<int, 1>{});
  }

  // ---- hand-over ----
  f32x4 bvs[FN];
  {
    const int ln = (lane >> 4) * 4;
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      const int n = wn0 + i * 16 + ln;
      bvs[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (a.bias) bvs[i] = *reinterpret_cast<const f32x4*>(a.bias + (long long)(n >> 6) * H + head * 64 + (n & 63));
    }
  }
  __syncthreads();   // the ring is dead
  char* const qkv = smem + RED_BYTES;   // [slot][Q | K | V][64 tokens][128 B]
  {
    constexpr int HALF = FN * FM / 2;
    f32x4* out_red = reinterpret_cast<f32x4*>(smem) + ((size_t)(group * NWC + gw) * HALF) * 64 + lane;
    const f32x4* in_red = reinterpret_cast<const f32x4*>(smem) + ((size_t)((group ^ 1) * NWC + gw) * HALF) * 64 + lane;
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FM; ++j)
        if (((i * FM + j) & 1) != group) out_red[((i * FM + j) >> 1) * 64] = acc[i][j];
    __syncthreads();
    const int lm = lane & 15, ln = (lane >> 4) * 4;
    char* const slot_base = qkv + (wm0 >> 6) * SLOT_B;
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      const int n = wn0 + i * 16 + ln, blk = n >> 6, d = n & 63;   // blk: 0 Q, 1 K, 2 V (uniform over the fragment)
      const f32x4 bv = bvs[i];
#pragma unroll
      for (int j = 0; j < FM; ++j) {
        if (((i * FM + j) & 1) != group) continue;
        const f32x4 v = acc[i][j] + in_red[((i * FM + j) >> 1) * 64] + bv;
        typename Vec4<T>::type o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = from_f32<T>(v[e]);
        const int tok = j * 16 + lm;
        const int swz = blk == 2 ? ((tok >> 1) & 1) << 2 : (tok >> 1) & 7;
        *reinterpret_cast<typename Vec4<T>::type*>(slot_base + blk * HEAD_B + tok * ROWB + (((d >> 3) ^ swz) << 4) + (d & 4) * 2) = o;
      }
    }
  }
  __syncthreads();   // Q, K, V of both slots are complete; the exchange area is dead

  // ---- phase 2 ----
  const int qblocks = (S + 31) >> 5;   // = KV tiles
  if (wave >= G * qblocks) return;     // (wave-uniform; no workgroup barrier from here on)
  const int slot = wave / qblocks, qb = wave - slot * qblocks;
  const int item = item0 + slot;
  if (item >= N) return;               // ragged last group
  const int q0 = qb * 32;
  char* const priv = smem + wave * PRIV_B;
  float* const wmask = reinterpret_cast<float*>(priv + PRIV_MASK);
  {
    float v = -INFINITY;
    if (lane < S) {
      const long long mv = a.mask ? a.mask[(long long)item * S + lane] : 1;
      v = (1.0f - (float)mv) * (-10000.0f * LOG2E);
    }
    wmask[lane] = v;
  }
  const char* const qt = qkv + slot * SLOT_B;
  int koff[4];
  {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) koff[s] = r * 128 + (((2 * s + h) ^ ((r >> 1) & 7)) << 4);
  }
  unsigned vlane[2];
  {
    const int g = lane >> 4, i = lane & 15, q4 = i >> 2, p = i & 3, h = lane >> 5;
    const int row = 4 * h + q4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int c = 4 * mt + 2 * (g & 1) + (p >> 1);
      const int pc = c ^ (((q4 >> 1) & 1) << 2);
      vlane[mt] = row * 128 + pc * 16 + (p & 1) * 8;
    }
  }
  V8 qf[4];   // rows past S hold the projection of token S - 1: attn_kernel's clamped query rows
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = lds_read8<T>(qt + q0 * ROWB + koff[s]);
  const unsigned v_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)(qt + 2 * HEAD_B);
  const float sl2 = a.scale * LOG2E;
  float m_run = -1e30f, l_run = 0.f;
  f32x16 ot[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { ot[0][i] = 0.f; ot[1][i] = 0.f; }
  const int h4 = 4 * (lane >> 5);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's mask row has landed (its LDS operations run in order)
  for (int t = 0; t < qblocks; ++t)
    attn_tile_step<T, true>(qt + HEAD_B + t * TILE_B, v_lds + t * TILE_B, koff, vlane, qf, wmask + t * KVT, t * KVT, S, sl2, h4, m_run, l_run, ot);

  // attn_kernel's merge of ONE partial, through the wave's own scratch
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  float* ow = reinterpret_cast<float*>(priv);
  float* mw = ow + 32 * OPAD;
  float* lw = mw + 32;
  {
    const int q = lane & 31;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        f32x4 v = {ot[mt][4 * g4], ot[mt][4 * g4 + 1], ot[mt][4 * g4 + 2], ot[mt][4 * g4 + 3]};
        *reinterpret_cast<f32x4*>(ow + q * OPAD + 32 * mt + 8 * g4 + h4) = v;
      }
    if (lane < 32) { mw[q] = m_run; lw[q] = l_tot; }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  for (int idx = lane; idx < 256; idx += 64) {
    const int q = idx >> 3, dc = idx & 7;
    const float M = fmaxf(-1e30f, mw[q]);
    const float wgt = __builtin_amdgcn_exp2f(mw[q] - M);
    const float L = 0.f + wgt * lw[q];
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(ow + q * OPAD + 8 * dc);
    const f32x4 x1 = *reinterpret_cast<const f32x4*>(ow + q * OPAD + 8 * dc + 4);
    float o[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[e] = 0.f + wgt * x0[e]; o[4 + e] = 0.f + wgt * x1[e]; }
    if (q0 + q >= S) continue;
    const float inv = 1.0f / L;
    V8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = from_f32<T>(o[e] * inv);
    T* op = (T*)a.O + ((long long)item * S + q0 + q) * H + head * 64 + 8 * dc;
    *reinterpret_cast<V8*>(op) = r;
  }
}

std::atomic<long long> g_qkv_attn_launches, g_attn_launches[2];
std::atomic<long long>& attn_launch_counter(bool masked) { return g_attn_launches[masked ? 1 : 0]; }

// Several prompts over one K/V stream.  Workgroup = (K/V item, head, group of 4 prompt slots, grid split); wave w owns the 32 queries of
// slot 4 group + w exactly as a wave of attn_kernel<T, false, 1> owns its unit (Q fragments in registers, own online softmax, no cross-wave
// merge).  The K/V tiles are staged once per workgroup: every wave fetches rows 8 w .. 8 w + 7 of each K and V tile of a stage by LDS-DMA
// (same K / V swizzles on the source address), all four read the whole stage.  Ring of SH_STAGES stages with one stage in flight across
// the barrier:
//   iteration s:  s_waitcnt vmcnt(own loads of stage s + 1 may stay in flight)   -> this wave's part of stage s has landed
//                 s_barrier                                                       -> every wave's part has, and every wave is done with s - 1
//                 issue stage s + 2 into the buffer of stage s - 1
//                 read + compute stage s
// The barrier is the raw one: __syncthreads() would drain the DMA in flight (vmcnt(0)).  Every LDS read of the loop is inline asm with its
// own lgkmcnt(0), so no read is pending when a wave arrives at the next barrier and hipcc has no LDS load to order behind the DMA.
// The spare waves of the last group (kv_share % 4 != 0) repeat the last slot: same loads, same barriers, no store.
template <typename T>
__global__ void __launch_bounds__(256) attn_shared_kernel(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int groups = (a.kv_share + 3) >> 2;
  const int ntiles_all = (a.kv_len + KVT - 1) / KVT;
  const int nstages_all = (ntiles_all + SH_TPS - 1) / SH_TPS;

  int b = blockIdx.x;
  const int gs = b % a.nsplit; b /= a.nsplit;
  const int grp = b % groups; b /= groups;
  const int head = b % a.heads;
  const int kv_item = b / a.heads;
  const int slot = grp * 4 + wave;
  const bool active = slot < a.kv_share;
  const int item = kv_item * a.kv_share + min(slot, a.kv_share - 1);

  const int sps = (nstages_all + a.nsplit - 1) / a.nsplit;  // stages per grid split
  const int sb = gs * sps;
  const int se = min(sb + sps, nstages_all);

  const T* Kb = (const T*)a.K + (long long)kv_item * a.k_item_stride + (long long)head * a.k_head_stride;
  const T* Vb = (const T*)a.V + (long long)kv_item * a.v_item_stride + (long long)head * a.v_head_stride;

  // ---- Q fragments (as attn_kernel) ----
  typename Vec8<T>::type qf[4];
  {
    const int qr = min(lane & 31, a.q_rows - 1);
    const T* qp = (const T*)a.Q + (long long)item * a.q_item_stride + (long long)qr * a.q_ld + head * 64 + 8 * (lane >> 5);
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const typename Vec8<T>::type*>(qp + 16 * s);
  }
  // the Q loads retire here, ahead of the first DMA: the counted waits below then count DMA only
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // ---- this wave's quarter of a stage: rows 8 wave + (lane >> 3) of every tile, physical chunk lane & 7 ----
  const int row = 8 * wave + (lane >> 3), sc = lane & 7;
  const int kc = sc ^ ((row >> 1) & 7);
  const int vc = sc ^ (((row >> 1) & 1) << 2);
  auto issue = [&](int buf, int s) {
    char* st = smem + buf * SH_STAGE_B + wave * 1024;
#pragma unroll
    for (int j = 0; j < SH_TPS; ++j) {
      const int tok = min((s * SH_TPS + j) * KVT + row, a.kv_len - 1);
      glds16((const char*)(Kb + (long long)tok * a.k_ld) + kc * 16, st + j * 2 * TILE_B);
      glds16((const char*)(Vb + (long long)tok * a.v_ld) + vc * 16, st + j * 2 * TILE_B + TILE_B);
    }
  };

  // ---- fragment read addresses (as attn_kernel) ----
  unsigned koff[4];
  {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) koff[s] = r * 128 + (((2 * s + h) ^ ((r >> 1) & 7)) << 4);
  }
  unsigned vlane[2];
  {
    const int g = lane >> 4, i = lane & 15, q4 = i >> 2, p = i & 3, h = lane >> 5;
    const int vrow = 4 * h + q4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int c = 4 * mt + 2 * (g & 1) + (p >> 1);
      const int pc = c ^ (((q4 >> 1) & 1) << 2);
      vlane[mt] = vrow * 128 + pc * 16 + (p & 1) * 8;
    }
  }
  const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;

  const float sl2 = a.scale * LOG2E;
  float m_run = -1e30f, l_run = 0.f;
  f32x16 ot[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { ot[0][i] = 0.f; ot[1][i] = 0.f; }
  const int h4 = 4 * (lane >> 5);

  if (sb < se) issue(0, sb);
  if (sb + 1 < se) issue(1, sb + 1);
  int buf = 0;
  for (int s = sb; s < se; ++s) {
    if (s + 1 < se) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * SH_TPS) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (s + 2 < se) issue(buf >= 1 ? buf - 1 : SH_STAGES - 1, s + 2);   // (buf + 2) % 3: the buffer stage s - 1 was read from

#pragma unroll
    for (int j = 0; j < SH_TPS; ++j) {
      const int t = s * SH_TPS + j;
      if (t >= ntiles_all) break;   // workgroup-uniform: the last stage of an odd tile count
      const unsigned kbase = smem_lds + buf * SH_STAGE_B + j * 2 * TILE_B;

      // S^T = K * Q^T
      i32x4v k0, k1, k2, k3;
      asm volatile(
          "ds_read_b128 %0, %4\n\t"
          "ds_read_b128 %1, %5\n\t"
          "ds_read_b128 %2, %6\n\t"
          "ds_read_b128 %3, %7\n\t"
          "s_waitcnt lgkmcnt(0)"
          : "=&v"(k0), "=&v"(k1), "=&v"(k2), "=&v"(k3)
          : "v"(kbase + koff[0]), "v"(kbase + koff[1]), "v"(kbase + koff[2]), "v"(kbase + koff[3])
          : "memory");
      f32x16 st;
#pragma unroll
      for (int i = 0; i < 16; ++i) st[i] = 0.f;
      st = mfma32<T>(__builtin_bit_cast(typename Vec8<T>::type, k0), qf[0], st);
      st = mfma32<T>(__builtin_bit_cast(typename Vec8<T>::type, k1), qf[1], st);
      st = mfma32<T>(__builtin_bit_cast(typename Vec8<T>::type, k2), qf[2], st);
      st = mfma32<T>(__builtin_bit_cast(typename Vec8<T>::type, k3), qf[3], st);

      // scores in log2 units, tail mask (as attn_kernel without an additive mask)
      const int tok0 = t * KVT;
      float mx = -INFINITY;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g4 + e;
          float y = st[i] * sl2;
          if (tok0 + 8 * g4 + h4 + e >= a.kv_len) y = -INFINITY;
          st[i] = y;
          mx = fmaxf(mx, y);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
      m_run = m_new;
      float psum = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = __builtin_amdgcn_exp2f(st[i] - m_new);
        st[i] = p;
        psum += p;
      }
      l_run = l_run * alpha + psum;
#pragma unroll
      for (int i = 0; i < 16; ++i) { ot[0][i] *= alpha; ot[1][i] *= alpha; }

      typename Vec8<T>::type pf[2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int e = 0; e < 8; ++e) pf[s2][e] = from_f32<T>(st[8 * s2 + e]);

      // O^T += V^T * P^T
      {
        const unsigned vaddr0 = kbase + TILE_B + vlane[0];
        const unsigned vaddr1 = kbase + TILE_B + vlane[1];
        i16x4 r00, r01, r02, r03, r10, r11, r12, r13;
        asm volatile(
            "ds_read_b64_tr_b16 %0, %8\n\t"
            "ds_read_b64_tr_b16 %1, %8 offset:1024\n\t"
            "ds_read_b64_tr_b16 %2, %8 offset:2048\n\t"
            "ds_read_b64_tr_b16 %3, %8 offset:3072\n\t"
            "ds_read_b64_tr_b16 %4, %9\n\t"
            "ds_read_b64_tr_b16 %5, %9 offset:1024\n\t"
            "ds_read_b64_tr_b16 %6, %9 offset:2048\n\t"
            "ds_read_b64_tr_b16 %7, %9 offset:3072\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(r00), "=&v"(r01), "=&v"(r02), "=&v"(r03), "=&v"(r10), "=&v"(r11), "=&v"(r12), "=&v"(r13)
            : "v"(vaddr0), "v"(vaddr1)
            : "memory");
        auto cat = [](i16x4 lo, i16x4 hi) {
          i16x8 v8;
          v8[0] = lo[0]; v8[1] = lo[1]; v8[2] = lo[2]; v8[3] = lo[3];
          v8[4] = hi[0]; v8[5] = hi[1]; v8[6] = hi[2]; v8[7] = hi[3];
          return __builtin_bit_cast(typename Vec8<T>::type, v8);
        };
        ot[0] = mfma32<T>(cat(r00, r01), pf[0], ot[0]);
        ot[0] = mfma32<T>(cat(r02, r03), pf[1], ot[0]);
        ot[1] = mfma32<T>(cat(r10, r11), pf[0], ot[1]);
        ot[1] = mfma32<T>(cat(r12, r13), pf[1], ot[1]);
      }
    }
    buf = buf + 1 == SH_STAGES ? 0 : buf + 1;
  }

  // ---- each wave finishes its own slot: O^T -> [q][d] through its own LDS region (the ring is idle behind the barrier) ----
  __syncthreads();
  const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
  float* ow = reinterpret_cast<float*>(smem + wave * SH_PARK_B);
  float* mw = ow + 32 * OPAD;
  float* lw = mw + 32;
  {
    const int q = lane & 31;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        f32x4 v = {ot[mt][4 * g4], ot[mt][4 * g4 + 1], ot[mt][4 * g4 + 2], ot[mt][4 * g4 + 3]};
        *reinterpret_cast<f32x4*>(ow + q * OPAD + 32 * mt + 8 * g4 + h4) = v;
      }
    if (lane < 32) { mw[q] = m_run; lw[q] = l_tot; }
  }
  __syncthreads();
  if (!active) return;
  const long long unit = (long long)item * a.heads + head;
  for (int idx = lane; idx < 256; idx += 64) {
    const int q = idx >> 3, dc = idx & 7;
    const float M = mw[q], L = lw[q];
    const f32x4 x0 = *reinterpret_cast<const f32x4*>(ow + q * OPAD + 8 * dc);
    const f32x4 x1 = *reinterpret_cast<const f32x4*>(ow + q * OPAD + 8 * dc + 4);
    if (a.nsplit > 1) {
      float* pp = a.part + (unit * a.nsplit + gs) * PART_STRIDE;
      *reinterpret_cast<f32x4*>(pp + q * 64 + 8 * dc) = x0;
      *reinterpret_cast<f32x4*>(pp + q * 64 + 8 * dc + 4) = x1;
      if (dc == 0) { pp[32 * 64 + q] = M; pp[32 * 64 + 32 + q] = L; }
    } else if (q < a.q_rows) {
      const float inv = 1.0f / L;
      typename Vec8<T>::type r;
#pragma unroll
      for (int e = 0; e < 4; ++e) { r[e] = from_f32<T>(x0[e] * inv); r[4 + e] = from_f32<T>(x1[e] * inv); }
      T* op = (T*)a.O + (long long)item * a.o_item_stride + (long long)q * a.o_ld + head * 64 + 8 * dc;
      *reinterpret_cast<typename Vec8<T>::type*>(op) = r;
    }
  }
}

template <typename T>
int launch_shared_t(const AttnArgs& a, hipStream_t stream) {
  const int groups = (a.kv_share + 3) / 4;
  const long long wgs = (long long)(a.items / a.kv_share) * a.heads * groups * a.nsplit;
  if (wgs > 0x7fffffffLL) return -1;
  hipLaunchKernelGGL(attn_shared_kernel<T>, dim3((unsigned)wgs), dim3(256), SH_LDS, stream, a);
  if (a.nsplit > 1) hipLaunchKernelGGL(attn_combine_kernel<T>, dim3(a.items * a.heads), dim3(256), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace

size_t attn_partial_bytes(int items, int heads, int q_rows, int nsplit) {
  if (nsplit <= 1) return 0;
  const int qblocks = (q_rows + 31) >> 5;
  return (size_t)items * heads * qblocks * nsplit * PART_STRIDE * sizeof(float);
}

int attn_pick_split(int items, int heads, int q_rows, int kv_len) {
  const int qblocks = (q_rows + 31) >> 5;
  const int nunits = items * heads * qblocks;
  const int ntiles = (kv_len + KVT - 1) / KVT;
  if (ntiles < 64) return 1;
  // two 64 KB workgroups fit a CU: aim for a multiple of 512 workgroups with >= 16 tiles each
  int best = 1;
  for (int s = 1; s <= 16; ++s) {
    if (ntiles / s < 16) break;
    best = s;
    if ((long long)nunits * s >= 1536) break;
  }
  return best;
}

int launch_attention(const AttnArgs& args, int op_dtype, hipStream_t stream) {
  AttnArgs a = args;
  if (a.kv_share < 1) a.kv_share = 1;   // (a zero-filled AttnArgs means what it always meant)
  if (a.items <= 0 || a.heads <= 0 || a.q_rows <= 0 || a.kv_len <= 0 || a.nsplit < 1) return -1;
  if (a.nsplit > 1 && !a.part) return -1;
  if ((a.q_ld | a.o_ld | a.k_ld | a.v_ld) & 7) return -1;  // 16-byte rows
  if (a.items % a.kv_share) return -1;
  return op_dtype == OP_F16 ? launch_t<f16>(a, stream) : launch_t<bf16>(a, stream);
}

bool qkv_attn_supported(int S, int H, int heads) { return S >= 1 && S <= 64 && heads >= 1 && H == heads * 64; }

int launch_qkv_attention(const void* X, const void* wqkv, const float* bqkv, const long long* mask, void* ctx, int N, int S, int H, int heads,
                         int op_dtype, hipStream_t stream) {
  if (N <= 0) return 0;
  if (!X || !wqkv || !ctx || !qkv_attn_supported(S, H, heads) || (op_dtype != OP_F16 && op_dtype != OP_BF16)) return -1;
  const long long groups = ((long long)N + 1) / 2;
  if (groups * heads > 0x7fffffffLL) return -1;
  const QkvAttnArgs a{X, wqkv, bqkv, mask, ctx, N, S, H, heads, 0.125f};
  constexpr size_t lds = 4 * (192 + 128) * 128;   // the ring: 4 slots of one 64-deep K tile of 192 weight + 128 activation rows, 160 KB
  const void* fn = op_dtype == OP_F16 ? (const void*)qkv_attn_kernel<f16> : (const void*)qkv_attn_kernel<bf16>;
  if (!ensure_lds(fn, lds)) return -3;
  const dim3 grid((unsigned)(groups * heads));
  if (op_dtype == OP_F16) hipLaunchKernelGGL(qkv_attn_kernel<f16>, grid, dim3(512), lds, stream, a);
  else hipLaunchKernelGGL(qkv_attn_kernel<bf16>, grid, dim3(512), lds, stream, a);
  if (hipGetLastError() != hipSuccess) return -4;
  g_qkv_attn_launches.fetch_add(1, std::memory_order_relaxed);
  return 0;
}
long long qkv_attn_launch_count() { return g_qkv_attn_launches.load(std::memory_order_relaxed); }
long long attn_launch_count(int masked) { return g_attn_launches[masked ? 1 : 0].load(std::memory_order_relaxed); }

int attn_shared_pick_split(int kv_items, int kv_share, int heads, int kv_len) {
  const int units = kv_items * heads * ((kv_share + 3) / 4);
  const int ntiles = (kv_len + KVT - 1) / KVT;
  const int nstages = (ntiles + SH_TPS - 1) / SH_TPS;
  if (ntiles < 64) return 1;   // the threshold of attn_pick_split: below it a second launch costs more than the idle CUs
  // three 48 KB workgroups fit a CU: split until 512 workgroups, each with >= 8 stages (16 tiles) behind its prologue
  int best = 1;
  for (int s = 1; s <= 16; ++s) {
    if (nstages / s < 8) break;
    best = s;
    if ((long long)units * s >= 512) break;
  }
  return best;
}

int launch_attention_shared(const AttnArgs& args, int op_dtype, hipStream_t stream) {
  AttnArgs a = args;
  if (a.items <= 0 || a.heads <= 0 || a.q_rows <= 0 || a.q_rows > 32 || a.kv_len <= 0 || a.nsplit < 1 || a.kv_share < 1) return -1;
  if (a.items % a.kv_share || a.mask || a.lse) return -1;
  if (a.nsplit > 1 && !a.part) return -1;
  if ((a.q_ld | a.o_ld | a.k_ld | a.v_ld) & 7) return -1;  // 16-byte rows
  return op_dtype == OP_F16 ? launch_shared_t<f16>(a, stream) : launch_shared_t<bf16>(a, stream);
}

}  // namespace mra
