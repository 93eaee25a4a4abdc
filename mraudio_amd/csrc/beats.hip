// BEATs audio encoder (row A1 / N4, the audio half): the callee of the reference's per-position loop, `audio_encoder(fbank)` at
// models/xinstructblip.py:267-275, built by LAVIS BeatsEncoder(checkpoint_path) (init_audio_encoder, :670-676), whose forward is
// BEATs' extract_features(fbank, padding_mask=None, feature_only=True)[0].  Neither source is vendored: the arithmetic is the
// published BEATs geometry restated by mraudio_amd/models/beats.py, whose transformer is pinned to transformers' WavLMEncoder
// (tests/test_beats.py, tests/golden/beats.npz; WavLM = BEATs with deep_norm_alpha 1 and the gate taken from the layer input).
//
// One batched forward over ALL chunks of a step ([n, F, 128] filterbanks -> [n, P, 768], P = F / 16 * 8):
//   patch gather -> patch GEMM -> LayerNorm(512) -> projection GEMM -> x += GELU(grouped positional convolution) -> LayerNorm
//   L x { QKV GEMM -> attention core with the gated relative-position bias -> out_proj GEMM + alpha x -> LayerNorm (-> alpha x)
//         -> fc1 GEMM + GELU -> fc2 GEMM + alpha x -> LayerNorm (-> alpha x) }
// The four GEMMs per layer run on gemm.hip's families with bias / GELU / residual fused.  Deep norm needs no GEMM epilogue of its own:
// the LayerNorm kernel writes both the f16 operand of the next GEMM and the fp32 stream PRE-MULTIPLIED by alpha, so the residual
// GEMM's `acc + bias + R` (R = C = the stream, updated in place) is `alpha x + y`.  The last LayerNorm writes the output unscaled.
// Precision follows the ViT: f16 MFMA operands, fp32 accumulation, residual stream, LayerNorm statistics and softmax.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "mra_common.h"
#include "mra_handle.h"

using namespace mra;
using namespace mra_host;

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int HD = 64;           // head dimension
constexpr int KV_PITCH = 144;    // LDS row pitch of K / V (bytes): 64 f16 + one 16-byte slot, conflict-free ds_read_b128 over 16 rows
constexpr int MAX_TOKENS = 512;  // K / V of one head at 512 tokens: 2 x 72 KB of LDS
constexpr int CG = 48;           // channels per group of the positional convolution (768 / 16)
constexpr int WIN_PITCH = 112;   // LDS row pitch of the convolution window (bytes): 48 f16 + one 16-byte slot

// ---------------------------------------------------------------------------------------------------------
// Patch gather: the 16 x 16 patches of the filterbank do not overlap, so the A operand of the patch GEMM is a permutation of
// the input (no im2col): row n * P + t * nf + f, column i * 16 + j  <-  fbank[n][16 t + i][16 f + j].  Eight elements per thread.
// ---------------------------------------------------------------------------------------------------------
template <typename TI>
__global__ void __launch_bounds__(256) beats_patch_kernel(const TI* fb, f16* A, long long total8, int F, int P, int mel, int ps) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total8) return;
  const int kp = ps * ps, per_row = kp / 8, nf = mel / ps;
  const long long row = idx / per_row;
  const int col = (int)(idx - row * per_row) * 8;
  const long long n = row / P;
  const int p = (int)(row - n * P), t = p / nf, f = p - t * nf;
  const int i = col / ps, j = col - i * ps;
  const TI* src = fb + (n * F + (long long)ps * t + i) * mel + ps * f + j;
  Vec8<f16>::type v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (f16)(float)src[e];
  *reinterpret_cast<Vec8<f16>::type*>(A + row * kp + col) = v;
}

// ---------------------------------------------------------------------------------------------------------
// LayerNorm of fp32 rows (H = 256 NC): one wave per row.  y16 = LN(x) in f16 (may be null), y32 = scale * LN(x) in fp32 (may be
// null; may alias x: the wave holds its row in registers before it writes).  The post-LN layers' deep norm: scale = alpha.
// ---------------------------------------------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(256) beats_ln_kernel(const float* x, long long rows, const float* g, const float* b, float eps, float scale,
                                                       float* y32, f16* y16) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  constexpr int H = 256 * NC;
  const float* xr = x + row * H;
  float4 v[NC];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    v[c] = *reinterpret_cast<const float4*>(xr + 256 * c + 4 * lane);
    s += v[c].x + v[c].y + v[c].z + v[c].w;
  }
  const float mu = wave_sum(s) * (1.0f / H);
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const float a = v[c].x - mu, bb = v[c].y - mu, cc = v[c].z - mu, d = v[c].w - mu;
    q += a * a + bb * bb + cc * cc + d * d;
  }
  const float rstd = rsqrtf(wave_sum(q) * (1.0f / H) + eps);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = 256 * c + 4 * lane;
    const float4 gg = *reinterpret_cast<const float4*>(g + col), bv = *reinterpret_cast<const float4*>(b + col);
    float4 y;
    y.x = (v[c].x - mu) * rstd * gg.x + bv.x;
    y.y = (v[c].y - mu) * rstd * gg.y + bv.y;
    y.z = (v[c].z - mu) * rstd * gg.z + bv.z;
    y.w = (v[c].w - mu) * rstd * gg.w + bv.w;
    if (y16) {
      Vec4<f16>::type h;
      h[0] = (f16)y.x; h[1] = (f16)y.y; h[2] = (f16)y.z; h[3] = (f16)y.w;
      *reinterpret_cast<Vec4<f16>::type*>(y16 + row * H + col) = h;
    }
    if (y32) {
      y.x *= scale; y.y *= scale; y.z *= scale; y.w *= scale;
      *reinterpret_cast<float4*>(y32 + row * H + col) = y;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Positional convolution as an implicit GEMM per (chunk, group): C[t][o] = sum_{k, c} x[t + k - pad][c] W[o][c][k] over the 48 channels
// of the group, M = tokens, N = 48, K = 48 x taps (6144).  The contraction index is kk = k * 48 + c (weights re-ordered to [o][kk] when
// loaded), so a lane's eight consecutive kk never straddle a tap and the A fragment of row t is ONE 16-byte LDS read at window row
// t + k, channel c: the window -- the chunk's tokens of this group, f16, with `pad` zero rows on either side -- is staged once and
// slides under the MFMAs.  Wave w owns tokens [64 w, 64 w + 64) x 48 outputs (4 x 3 fragments of 16 x 16); the weight fragments come
// straight from L2 (one group's 590 KB is shared by every workgroup of that group).  Epilogue: x[t][o] += GELU(acc + bias), in place
// (this workgroup is the only reader and writer of its (chunk, group) block, and it staged that block before the first store).
// ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(512) beats_posconv_kernel(float* x, const f16* W, const float* bias, int P, int D, int taps, int groups) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int item = blockIdx.x / groups, grp = blockIdx.x - item * groups;
  const int pad = taps / 2;
  const int nw = (P + 63) / 64;
  const int wrows = nw * 64 + taps - 1;        // covers every row any wave's fragments read
  float* xi = x + (long long)item * P * D + grp * CG;
  for (int c = tid; c < wrows * (CG / 8); c += 512) {
    const int r = c / (CG / 8), ch = c - r * (CG / 8);
    const int t = r - pad;
    Vec8<f16>::type v;
    if (t >= 0 && t < P) {
      const float4 a = *reinterpret_cast<const float4*>(xi + (long long)t * D + ch * 8);
      const float4 b = *reinterpret_cast<const float4*>(xi + (long long)t * D + ch * 8 + 4);
      v[0] = (f16)a.x; v[1] = (f16)a.y; v[2] = (f16)a.z; v[3] = (f16)a.w; v[4] = (f16)b.x; v[5] = (f16)b.y; v[6] = (f16)b.z; v[7] = (f16)b.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (f16)0.f;
    }
    *reinterpret_cast<Vec8<f16>::type*>(smem + r * WIN_PITCH + ch * 16) = v;
  }
  __syncthreads();
  if (wave >= nw) return;
  using V8 = Vec8<f16>::type;
  const int lm = lane & 15, lc = lane >> 4;
  const int row0 = wave * 64;
  const int KK = CG * taps;
  const f16* wb = W + ((long long)grp * CG + lm) * KK + 8 * lc;
  f32x4 acc[4][3];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int nn = 0; nn < 3; ++nn) acc[m][nn] = f32x4{0.f, 0.f, 0.f, 0.f};
  const char* ab = smem + (row0 + lm) * WIN_PITCH;
  V8 bcur[3];
#pragma unroll
  for (int nn = 0; nn < 3; ++nn) bcur[nn] = *reinterpret_cast<const V8*>(wb + (long long)16 * nn * KK);
  for (int s = 0; s < KK / 32; ++s) {
    const int kk = 32 * s + 8 * lc;
    const int k = kk / CG, c = kk - k * CG;
    V8 bnext[3];
    const int sn = s + 1 < KK / 32 ? s + 1 : s;
#pragma unroll
    for (int nn = 0; nn < 3; ++nn) bnext[nn] = *reinterpret_cast<const V8*>(wb + (long long)16 * nn * KK + 32 * sn);
    const char* ap = ab + k * WIN_PITCH + c * 2;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const V8 af = *reinterpret_cast<const V8*>(ap + 16 * m * WIN_PITCH);
#pragma unroll
      for (int nn = 0; nn < 3; ++nn) acc[m][nn] = mfma16<f16>(af, bcur[nn], acc[m][nn]);
    }
#pragma unroll
    for (int nn = 0; nn < 3; ++nn) bcur[nn] = bnext[nn];
  }
  // D: column = output channel 16 nn + lm, row = token 16 m + 4 lc + e
#pragma unroll
  for (int nn = 0; nn < 3; ++nn) {
    const int o = 16 * nn + lm;
    const float bo = bias[grp * CG + o];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int t = row0 + 16 * m + 4 * lc + e;
        if (t < P) xi[(long long)t * D + o] += gelu_erf(acc[m][nn][e] + bo);
      }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Attention core with the gated relative-position bias: one workgroup of eight waves per (chunk, head).  K and V of the head are
// staged once in LDS (S <= 512 tokens: 2 x 72 KB), with the head's bias column E[bucket(r)][h] * log2(e) for every distance
// r = j - i (the int16 bucket table comes from the host, computed there with torch's exact formula: no log on the GPU), and the
// head's gate projection (grep_linear, 8 x 64).  No [S, S] bias is materialised.  Each wave takes 16-query blocks; S^T = K Q^T puts
// the keys on the MFMA row index (as vit_attn_kernel), so a lane holds, for its query, keys 16 i + 4 c + 0..3 of every fragment i;
// the scores of a 128-key chunk stay in registers (online softmax across chunks), and fragments 2 ks and 2 ks + 1 are the B operand
// of K step ks of O^T = V^T P^T.
// The gate of a query row is computed here from the row's head slice of `gsrc` (the Q projection for BEATs, the layer input for
// WavLM): each of the four lanes of a query holds 16 of its 64 elements, forms partial sums of the eight projections, and two lane
// swaps complete them.  score = (q . k) / 8 + G[i] E[bucket(j - i)]; softmax in fp32 (exp2 units).
// ---------------------------------------------------------------------------------------------------------
template <int KP>
__global__ void __launch_bounds__(512) beats_attn_kernel(const f16* qkv, const f16* gsrc, int g_ld, const float* E, const short* bucket,
                                                         const float* gw, const float* gb, const float* ga, f16* ctx, int S, int heads) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;
  char* Vs = Ks + KP * KV_PITCH;
  float* Eb = reinterpret_cast<float*>(Vs + KP * KV_PITCH);   // [2 KP]: distance r = j - i at Eb[r + S - 1]
  float* Gw = Eb + 2 * KP;                                      // [8][64] then the 8 biases
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int item = blockIdx.x / heads, head = blockIdx.x - item * heads;
  const int D = heads * HD, ld = 3 * D;
  const f16* base = qkv + (long long)item * S * ld + head * HD;
  using V8 = Vec8<f16>::type;
  for (int c = tid; c < KP * 8; c += 512) {
    const int row = c >> 3, ch = c & 7;
    V8 kv, vv;
    if (row < S) {
      kv = *reinterpret_cast<const V8*>(base + (long long)row * ld + D + ch * 8);
      vv = *reinterpret_cast<const V8*>(base + (long long)row * ld + 2 * D + ch * 8);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) { kv[e] = (f16)0.f; vv[e] = (f16)0.f; }
    }
    *reinterpret_cast<V8*>(Ks + row * KV_PITCH + ch * 16) = kv;
    *reinterpret_cast<V8*>(Vs + row * KV_PITCH + ch * 16) = vv;
  }
  for (int r = tid; r < 2 * KP; r += 512) Eb[r] = r < 2 * S - 1 ? E[bucket[r] * heads + head] * LOG2E : 0.f;
  for (int r = tid; r < 8 * HD + 8; r += 512) Gw[r] = r < 8 * HD ? gw[r] : gb[r - 8 * HD];
  __syncthreads();
  const float gconst = ga[head];
  const float sl2 = LOG2E * 0.125f;   // 1 / sqrt(64), in exp2 units
  const int lm = lane & 15, lc = lane >> 4;
  const int nblocks = (S + 15) >> 4;
  const f16* gbase = gsrc + (long long)item * S * g_ld + head * HD;
  for (int qb = wave; qb < nblocks; qb += 8) {
    const int q0 = qb * 16;
    const int q = min(q0 + lm, S - 1);
    V8 qf[2], sf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[ks] = *reinterpret_cast<const V8*>(base + (long long)q * ld + 32 * ks + 8 * lc);
      sf[ks] = *reinterpret_cast<const V8*>(gbase + (long long)q * g_ld + 32 * ks + 8 * lc);
    }
    // gate: u[j] = sum_d gw[j][d] s[d] + gb[j]; this lane holds d = 32 ks + 8 lc + e
    float u[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = 0.f;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) a = fmaf(Gw[j * HD + 32 * ks + 8 * lc + e], (float)sf[ks][e], a);
      a += __shfl_xor(a, 16);
      a += __shfl_xor(a, 32);
      u[j] = a + Gw[8 * HD + j];
    }
    const float ua = 1.0f / (1.0f + __expf(-(u[0] + u[1] + u[2] + u[3])));
    const float ub = 1.0f / (1.0f + __expf(-(u[4] + u[5] + u[6] + u[7])));
    const float G = ua * (ub * gconst - 1.0f) + 2.0f;
    const float* eq = Eb + (S - 1 - q);   // eq[key] = bias of distance key - q (log2 units)
    // online softmax over chunks of 128 keys: eight score fragments live at a time (all 32 of S = 512 spill)
    float mx = -3.0e38f, l = 0.f;
    f32x4 ot[HD / 16];
#pragma unroll
    for (int df = 0; df < HD / 16; ++df) ot[df] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < S; k0 += 128) {
      f32x4 sc[8];
      float cm = -3.0e38f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int kb = k0 + 16 * i;
        if (kb >= S) { sc[i] = f32x4{-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f}; continue; }
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          const V8 kf = *reinterpret_cast<const V8*>(Ks + (kb + lm) * KV_PITCH + (4 * ks + lc) * 16);
          a = mfma16<f16>(kf, qf[ks], a);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int key = kb + 4 * lc + e;
          a[e] = key < S ? fmaf(a[e], sl2, G * eq[key]) : -3.0e38f;
          cm = fmaxf(cm, a[e]);
        }
        sc[i] = a;
      }
      cm = fmaxf(cm, __shfl_xor(cm, 16));
      cm = fmaxf(cm, __shfl_xor(cm, 32));
      const float mn = fmaxf(mx, cm);
      const float corr = __builtin_amdgcn_exp2f(mx - mn);   // first chunk: exp2(-huge) = 0 against zero accumulators
      mx = mn;
      l *= corr;
#pragma unroll
      for (int df = 0; df < HD / 16; ++df)
#pragma unroll
        for (int e = 0; e < 4; ++e) ot[df][e] *= corr;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (k0 + 32 * ks >= S) continue;
        V8 pf;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          pf[e] = (f16)__builtin_amdgcn_exp2f(sc[2 * ks][e] - mx);          // masked keys: exp2(-huge) = 0
          pf[4 + e] = (f16)__builtin_amdgcn_exp2f(sc[2 * ks + 1][e] - mx);
          l += (float)pf[e] + (float)pf[4 + e];
        }
        // V^T fragment in the same key order: transposed 4 x 16 blocks at keys 32 ks + 4 lc and 32 ks + 16 + 4 lc (rows < KP: zero past S)
        const char* vb = Vs + (k0 + 32 * ks + 4 * lc + (lm >> 2)) * KV_PITCH + (lane & 3) * 8;
#pragma unroll
        for (int df = 0; df < HD / 16; ++df) {
          const i16x4 c0 = lds_read_tr4(vb + df * 32), c1 = lds_read_tr4(vb + df * 32 + 16 * KV_PITCH);
          i16x8 v;
          v[0] = c0[0]; v[1] = c0[1]; v[2] = c0[2]; v[3] = c0[3]; v[4] = c1[0]; v[5] = c1[1]; v[6] = c1[2]; v[7] = c1[3];
          ot[df] = mfma16<f16>(__builtin_bit_cast(V8, v), pf, ot[df]);
        }
      }
    }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const float inv = 1.0f / l;
    if (q0 + lm < S) {
      f16* crow = ctx + ((long long)item * S + q0 + lm) * D + head * HD;
#pragma unroll
      for (int df = 0; df < HD / 16; ++df) {
        Vec4<f16>::type o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (f16)(ot[df][e] * inv);
        *reinterpret_cast<Vec4<f16>::type*>(crow + 16 * df + 4 * lc) = o;
      }
    }
  }
}

// effective positional-convolution weight [o][c][k] (any dtype) -> the implicit GEMM's [o][k * cg + c] in f16
template <typename TI>
__global__ void __launch_bounds__(256) beats_convw_kernel(const TI* src, f16* dst, int D, int cg, int taps) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)D * cg * taps) return;
  const long long o = idx / (cg * taps);
  const int r = (int)(idx - o * cg * taps), c = r / taps, k = r - c * taps;
  dst[o * cg * taps + (long long)k * cg + c] = (f16)(float)src[idx];
}

struct BeatsLayer {
  void *wqkv, *wout, *wfc1, *wfc2;
  float *bqkv, *bout, *bfc1, *bfc2;
  float *ln1g, *ln1b, *ln2g, *ln2b;
  float *gw, *gb, *ga;
};

}  // namespace

struct mra_beats {
  mra_beats_cfg cfg;
  int device = 0;
  char* arena = nullptr;
  size_t arena_bytes = 0;
  Registry params;   // every accepted parameter name (beats_layout)
  void *wpatch = nullptr, *wproj = nullptr, *wconv = nullptr;
  float *lnpg = nullptr, *lnpb = nullptr, *bproj = nullptr, *bconv = nullptr, *lneg = nullptr, *lneb = nullptr, *E = nullptr;
  std::vector<BeatsLayer> layers;
  std::map<int, short*> buckets;       // sequence length -> device int16 table [2 S - 1] of bucket(r - S + 1)
  int gemm_persist = 1;
};

namespace {

constexpr int BEATS_CONVW = 1;   // Param::store: [o][c][k] -> f16 [o][k * 48 + c] (beats_convw_kernel); 0 = plain conversion

// Lays the parameter arena out and registers every accepted name; with base == nullptr only measures.
size_t beats_layout(mra_beats* h, char* base) {
  const mra_beats_cfg& c = h->cfg;
  const size_t D = c.dim, I = c.ffn, Em = c.embed_dim, kp = (size_t)c.patch * c.patch;
  Carver cv(base);
  auto reg = [&](const std::string& name, void* p, int dtype, long long numel, bool required = true, int store = 0) {
    Param pr;
    pr.ptr = p; pr.dtype = dtype; pr.numel = numel; pr.required = required; pr.store = store;
    h->params[name] = pr;
  };
  auto w16 = [&](const std::string& name, void* p, long long numel) { reg(name, p, MRA_F16, numel); };
  auto f32 = [&](const std::string& name, float* p, long long numel, bool required = true) { reg(name, p, MRA_F32, numel, required); };
  h->wpatch = cv.take<char>(Em * kp, 2);
  h->lnpg = cv.take<float>(Em); h->lnpb = cv.take<float>(Em);
  h->wproj = cv.take<char>(D * Em, 2); h->bproj = cv.take<float>(D);
  h->wconv = cv.take<char>(D * (D / c.conv_pos_groups) * c.conv_pos, 2); h->bconv = cv.take<float>(D);
  h->lneg = cv.take<float>(D); h->lneb = cv.take<float>(D);
  h->E = cv.take<float>((size_t)c.num_buckets * c.heads);
  w16("patch_embedding.weight", h->wpatch, Em * kp);
  f32("layer_norm.weight", h->lnpg, Em); f32("layer_norm.bias", h->lnpb, Em);
  w16("post_extract_proj.weight", h->wproj, D * Em); f32("post_extract_proj.bias", h->bproj, D);
  reg("encoder.pos_conv.0.weight", h->wconv, MRA_F16, D * CG * c.conv_pos, true, BEATS_CONVW); f32("encoder.pos_conv.0.bias", h->bconv, D);
  f32("encoder.layer_norm.weight", h->lneg, D); f32("encoder.layer_norm.bias", h->lneb, D);
  f32("encoder.layers.0.self_attn.relative_attention_bias.weight", h->E, (long long)c.num_buckets * c.heads);
  h->layers.assign(c.layers, BeatsLayer{});
  for (int li = 0; li < c.layers; ++li) {
    BeatsLayer& L = h->layers[li];
    const std::string p = "encoder.layers." + std::to_string(li) + ".";
    L.wqkv = cv.take<char>(3 * D * D, 2); L.bqkv = cv.take<float>(3 * D);
    L.wout = cv.take<char>(D * D, 2); L.bout = cv.take<float>(D);
    L.wfc1 = cv.take<char>(I * D, 2); L.bfc1 = cv.take<float>(I);
    L.wfc2 = cv.take<char>(D * I, 2); L.bfc2 = cv.take<float>(D);
    L.ln1g = cv.take<float>(D); L.ln1b = cv.take<float>(D); L.ln2g = cv.take<float>(D); L.ln2b = cv.take<float>(D);
    L.gw = cv.take<float>(8 * HD); L.gb = cv.take<float>(8); L.ga = cv.take<float>(c.heads);
    const char* qkv[3] = {"q_proj", "k_proj", "v_proj"};
    for (int j = 0; j < 3; ++j) {   // into the packed Q | K | V weight and bias; a checkpoint may lack k_proj.bias (it stays zero)
      w16(p + "self_attn." + qkv[j] + ".weight", L.wqkv ? (char*)L.wqkv + j * D * D * 2 : nullptr, D * D);
      f32(p + "self_attn." + qkv[j] + ".bias", L.bqkv ? L.bqkv + j * D : nullptr, D, j != 1);
    }
    w16(p + "self_attn.out_proj.weight", L.wout, D * D); f32(p + "self_attn.out_proj.bias", L.bout, D);
    f32(p + "self_attn.grep_linear.weight", L.gw, 8 * HD); f32(p + "self_attn.grep_linear.bias", L.gb, 8); f32(p + "self_attn.grep_a", L.ga, c.heads);
    f32(p + "self_attn_layer_norm.weight", L.ln1g, D); f32(p + "self_attn_layer_norm.bias", L.ln1b, D);
    w16(p + "fc1.weight", L.wfc1, I * D); f32(p + "fc1.bias", L.bfc1, I);
    w16(p + "fc2.weight", L.wfc2, D * I); f32(p + "fc2.bias", L.bfc2, D);
    f32(p + "final_layer_norm.weight", L.ln2g, D); f32(p + "final_layer_norm.bias", L.ln2b, D);
  }
  return cv.off;
}

// torch's _relative_positions_bucket, operation for operation in float32 (r = key - query)
int bucket_of(int r, int num_buckets, int max_distance) {
  const int nb = num_buckets / 2;
  int out = r > 0 ? nb : 0;
  const int a = r < 0 ? -r : r;
  const int max_exact = nb / 2;
  if (a < max_exact) return out + a;
  float v = logf((float)a / (float)max_exact);
  v = v / (float)std::log((double)max_distance / max_exact);
  v = v * (float)(nb - max_exact);
  long long big = (long long)((float)max_exact + v);
  if (big > nb - 1) big = nb - 1;
  return out + (int)big;
}

int ln_rows(const float* x, long long rows, int H, const float* g, const float* b, float eps, float scale, float* y32, f16* y16, hipStream_t st) {
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  switch (H) {
    case 256: hipLaunchKernelGGL(beats_ln_kernel<1>, grid, block, 0, st, x, rows, g, b, eps, scale, y32, y16); break;
    case 512: hipLaunchKernelGGL(beats_ln_kernel<2>, grid, block, 0, st, x, rows, g, b, eps, scale, y32, y16); break;
    case 768: hipLaunchKernelGGL(beats_ln_kernel<3>, grid, block, 0, st, x, rows, g, b, eps, scale, y32, y16); break;
    case 1024: hipLaunchKernelGGL(beats_ln_kernel<4>, grid, block, 0, st, x, rows, g, b, eps, scale, y32, y16); break;
    default: return -1;
  }
  return 0;
}

size_t attn_lds_bytes(int kp) { return (size_t)2 * kp * KV_PITCH + (2 * kp + 8 * HD + 8) * sizeof(float); }
size_t conv_lds_bytes(int P, int taps) { return (size_t)(((P + 63) / 64) * 64 + taps - 1) * WIN_PITCH; }

}  // namespace

extern "C" {

void mra_beats_cfg_default(mra_beats_cfg* c) {
  c->dim = 768; c->heads = 12; c->ffn = 3072; c->layers = 12; c->embed_dim = 512; c->patch = 16; c->mel_bins = 128;
  c->conv_pos = 128; c->conv_pos_groups = 16; c->num_buckets = 320; c->max_distance = 800; c->ln_eps = 1e-5f;
  c->deep_norm_alpha = powf(2.0f * 12, 0.25f); c->gate_from = MRA_BEATS_GATE_Q; c->op_dtype = MRA_F16;
}

int mra_beats_create(const mra_beats_cfg* cfg, mra_beats** out) {
  if (!cfg || !out) return fail(MRA_EINVAL, "null argument");
  const mra_beats_cfg& c = *cfg;
  if (c.heads <= 0 || c.dim != c.heads * HD || c.dim % 256 || c.dim > 1024) return fail(MRA_EINVAL, "dim must be heads * 64, a multiple of 256, <= 1024");
  if (c.ffn <= 0 || c.ffn % 256 || c.layers <= 0) return fail(MRA_EINVAL, "ffn must be a multiple of 256; layers > 0");
  if (c.embed_dim <= 0 || c.embed_dim % 256 || c.embed_dim > c.dim) return fail(MRA_EINVAL, "embed_dim must be a multiple of 256, <= dim");
  if (c.patch <= 0 || c.patch % 8 || (c.patch * c.patch) % 64 || c.mel_bins <= 0 || c.mel_bins % c.patch) return fail(MRA_EINVAL, "patch must be a multiple of 8 dividing mel_bins");
  if (c.conv_pos_groups <= 0 || c.dim % c.conv_pos_groups || c.dim / c.conv_pos_groups != CG) return fail(MRA_EINVAL, "dim / conv_pos_groups must be 48");
  if (c.conv_pos <= 0 || c.conv_pos % 2 || (CG * c.conv_pos) % 32 || c.conv_pos > 256) return fail(MRA_EINVAL, "conv_pos must be even, <= 256, 48 * conv_pos a multiple of 32");
  if (c.num_buckets < 4 || c.num_buckets % 2 || c.max_distance <= c.num_buckets / 4) return fail(MRA_EINVAL, "bad relative-position buckets");
  if (c.gate_from != MRA_BEATS_GATE_Q && c.gate_from != MRA_BEATS_GATE_INPUT) return fail(MRA_EINVAL, "gate_from must be MRA_BEATS_GATE_Q or MRA_BEATS_GATE_INPUT");
  if (!(c.deep_norm_alpha > 0.f) || !(c.ln_eps > 0.f)) return fail(MRA_EINVAL, "deep_norm_alpha and ln_eps must be positive");
  if (c.op_dtype != MRA_F16) return fail(MRA_EINVAL, "op_dtype must be MRA_F16");
  mra_beats* h = new mra_beats();
  h->cfg = c;
  const int rc = create_arena(h, beats_layout, "BEATs");   // an absent k_proj.bias stays zero
  if (rc) { mra_beats_destroy(h); return rc; }
  *out = h;
  return MRA_OK;
}

void mra_beats_destroy(mra_beats* h) {
  if (!h) return;
  for (auto& kv : h->buckets) (void)hipFree(kv.second);
  if (h->arena) (void)hipFree(h->arena);
  delete h;
}

int mra_beats_load(mra_beats* h, const char* name, const void* src, int32_t dtype, const int64_t* shape, int32_t ndim, void* stream_) {
  if (!h || !name || !src || (ndim > 0 && !shape)) return fail(MRA_EINVAL, "null argument");
  if (dtype < MRA_F32 || dtype > MRA_BF16) return fail(MRA_EINVAL, "bad dtype");
  const mra_beats_cfg& c = h->cfg;
  hipStream_t st = as_stream(stream_);
  const std::string key(name);
  if (key == "encoder.pos_conv.0.weight_g" || key == "encoder.pos_conv.0.weight_v")
    return fail(MRA_ENAME, key + ": load the effective weight encoder.pos_conv.0.weight (weight norm folded by the caller)");
  Param* pr = find_param(h->params, key, "encoder.layers.", c.layers);
  if (!pr) return MRA_ENAME;
  int rc = check_numel(key, *pr, shape, ndim);
  if (rc) return rc;
  if (pr->store == BEATS_CONVW) {
    const dim3 grid((unsigned)((pr->numel + 255) / 256)), block(256);
    with_src(dtype, [&](auto ti) {
      using TI = decltype(ti);
      hipLaunchKernelGGL(beats_convw_kernel<TI>, grid, block, 0, st, (const TI*)src, (f16*)pr->ptr, c.dim, CG, c.conv_pos);
    });
    rc = hipGetLastError() == hipSuccess ? 0 : -4;
  } else {
    rc = launch_convert(src, dtype, pr->ptr, pr->dtype, pr->numel, st);
  }
  if (rc) return chk(rc, "beats load");
  pr->loaded = true;
  return MRA_OK;
}

int mra_beats_set_option(mra_beats* h, const char* name, int32_t value) {
  if (!h || !name) return fail(MRA_EINVAL, "null argument");
  const std::string key(name);
  if (key == "gemm_persist") {
    if (value != 0 && value != 1) return fail(MRA_EINVAL, "gemm_persist: 0 or 1");
    h->gemm_persist = value;
    return MRA_OK;
  }
  return fail(MRA_ENAME, "unknown option: " + key);
}

int mra_beats_missing(mra_beats* h) {
  if (!h) return -1;
  return count_missing(h->params);
}

namespace {
int beats_tokens(const mra_beats_cfg& c, int frames) { return frames / c.patch * (c.mel_bins / c.patch); }
// workspace: the f16 operand rows (a16), the wide f16 buffer (patches, Q | K | V, fc1 activation), the attention output (ctx)
size_t beats_ws_parts(const mra_beats* h, size_t M, size_t* a16, size_t* big) {
  const mra_beats_cfg& c = h->cfg;
  *a16 = align_up(M * c.dim * 2);
  *big = align_up(M * std::max<size_t>(std::max<size_t>(3 * c.dim, c.ffn), (size_t)c.patch * c.patch) * 2);
  return *a16 + *big + align_up(M * c.dim * 2) + 4096;
}
// What the two stages below need before their first launch at P tokens: the int16 bucket table of this sequence length (computed once per
// handle and length, exactly as torch computes it: the handle's one allocation after create) and the kernels' dynamic LDS.  Neither is a
// stream operation.
int beats_stage_prepare(mra_beats* h, int P, short** bucket = nullptr) {
  const mra_beats_cfg& c = h->cfg;
  auto it = h->buckets.find(P);
  if (it == h->buckets.end()) {
    std::vector<short> tab(2 * P - 1);
    for (int r = 0; r < 2 * P - 1; ++r) tab[r] = (short)bucket_of(r - (P - 1), c.num_buckets, c.max_distance);
    short* dev = nullptr;
    HIP_TRY(hipMalloc((void**)&dev, tab.size() * sizeof(short)));
    const hipError_t e = hipMemcpy(dev, tab.data(), tab.size() * sizeof(short), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(dev); return fail(MRA_EHIP, std::string("hipMemcpy of the bucket table: ") + hipGetErrorString(e)); }
    it = h->buckets.emplace(P, dev).first;
  }
  if (bucket) *bucket = it->second;
  if (!ensure_lds((const void*)beats_attn_kernel<256>, attn_lds_bytes(256)) || !ensure_lds((const void*)beats_attn_kernel<512>, attn_lds_bytes(512)) ||
      !ensure_lds((const void*)beats_posconv_kernel, conv_lds_bytes(MAX_TOKENS, 256)))
    return fail(MRA_EHIP, "hipFuncSetAttribute(beats kernels)");
  return MRA_OK;
}

// x [n * P][dim] fp32 += GELU(grouped positional convolution of x), in place: the launch of mra_beats_forward and mra_debug_beats_posconv.
int beats_posconv(mra_beats* h, float* x, int n, int P, hipStream_t st) {
  const mra_beats_cfg& c = h->cfg;
  const int rc = beats_stage_prepare(h, P);
  if (rc) return rc;
  hipLaunchKernelGGL(beats_posconv_kernel, dim3((unsigned)(n * c.conv_pos_groups)), dim3(512), conv_lds_bytes(P, c.conv_pos), st, x, (const f16*)h->wconv,
                     h->bconv, P, c.dim, c.conv_pos, c.conv_pos_groups);
  return MRA_OK;
}

// The attention core of layer L over n chunks of P tokens: qkv [n * P][3 dim] -> ctx [n * P][dim] (f16).  Owns the choice of the KP instantiation
// (256 keys of LDS up to P = 256, 512 above), the gate's source (the q third of qkv for BEATs; `layer_in` [n * P][dim], the layer input, for
// WavLM) and the bucket table: the launch of mra_beats_forward and mra_debug_beats_attention.
int beats_attention(mra_beats* h, const BeatsLayer& L, const f16* qkv, const f16* layer_in, int n, int P, f16* ctx, hipStream_t st) {
  const mra_beats_cfg& c = h->cfg;
  short* bucket = nullptr;
  const int rc = beats_stage_prepare(h, P, &bucket);
  if (rc) return rc;
  const int D = c.dim;
  const int KPt = P <= 256 ? 256 : 512;
  const size_t alds = attn_lds_bytes(KPt);
  const f16* gsrc = c.gate_from == MRA_BEATS_GATE_Q ? qkv : layer_in;
  const int g_ld = c.gate_from == MRA_BEATS_GATE_Q ? 3 * D : D;
  if (KPt == 256)
    hipLaunchKernelGGL(beats_attn_kernel<256>, dim3((unsigned)(n * c.heads)), dim3(512), alds, st, qkv, gsrc, g_ld, (const float*)h->E,
                       (const short*)bucket, (const float*)L.gw, (const float*)L.gb, (const float*)L.ga, ctx, P, c.heads);
  else
    hipLaunchKernelGGL(beats_attn_kernel<512>, dim3((unsigned)(n * c.heads)), dim3(512), alds, st, qkv, gsrc, g_ld, (const float*)h->E,
                       (const short*)bucket, (const float*)L.gw, (const float*)L.gb, (const float*)L.ga, ctx, P, c.heads);
  return MRA_OK;
}

bool beats_loaded(const mra_beats* h, std::initializer_list<std::string> names) {
  for (const std::string& k : names) {
    auto it = h->params.find(k);
    if (it == h->params.end() || !it->second.loaded) return false;
  }
  return true;
}
}  // namespace

size_t mra_beats_workspace_bytes(mra_beats* h, int32_t n, int32_t frames) {
  if (!h || n <= 0 || frames <= 0) return 0;
  const int P = beats_tokens(h->cfg, frames);
  if (P <= 0 || P > MAX_TOKENS) return 0;
  size_t a16, big;
  return beats_ws_parts(h, (size_t)n * P, &a16, &big);
}

int mra_beats_forward(mra_beats* h, const void* fbank, int32_t dtype, int32_t n, int32_t frames, void* out_, void* workspace, size_t workspace_bytes,
                      void* stream_) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (n < 0 || frames < 0) return fail(MRA_EINVAL, "negative chunk or frame count");
  if (n == 0) return MRA_OK;
  if (!fbank || !out_ || !workspace) return fail(MRA_EINVAL, "null argument");
  if (dtype != MRA_F32 && dtype != MRA_F16) return fail(MRA_EINVAL, "fbank must be f32 or f16");
  if (mra_beats_missing(h) > 0) return fail(MRA_ESTATE, std::to_string(mra_beats_missing(h)) + " BEATs parameters not loaded");
  const mra_beats_cfg& c = h->cfg;
  const int P = beats_tokens(c, frames);
  if (P <= 0 || P > MAX_TOKENS) return fail(MRA_EINVAL, "tokens per chunk must be in [1, 512]: frames / patch * mel_bins / patch = " + std::to_string(P));
  const long long M = (long long)n * P;
  if (M * std::max(3 * c.dim, c.ffn) > 0x7fffffffLL) return fail(MRA_EINVAL, "too many chunks for one call: split them");
  if (workspace_bytes < mra_beats_workspace_bytes(h, n, frames)) return fail(MRA_ENOMEM, "workspace too small: need " + std::to_string(mra_beats_workspace_bytes(h, n, frames)));
  if (reinterpret_cast<uintptr_t>(workspace) % 256) return fail(MRA_EINVAL, "workspace must be 256-byte aligned");
  const int D = c.dim, I = c.ffn, Em = c.embed_dim, kp = c.patch * c.patch;
  hipStream_t st = as_stream(stream_);
  size_t a16b, bigb;
  beats_ws_parts(h, (size_t)M, &a16b, &bigb);
  f16* a16 = (f16*)workspace;
  f16* big = (f16*)((char*)workspace + a16b);
  f16* ctx = (f16*)((char*)workspace + a16b + bigb);
  float* x = (float*)out_;   // the fp32 stream IS the output (the patch GEMM's [M, 512] rows pass through it first)
  int rc;
  if ((rc = beats_stage_prepare(h, P))) return rc;   // the bucket table of this sequence length and the kernels' LDS, before the first launch
  {   // front end: patches -> [M, 512] -> LayerNorm -> projection -> x
    const long long total8 = M * kp / 8;
    const dim3 grid((unsigned)((total8 + 255) / 256)), block(256);
    with_f32_f16(dtype, [&](auto ti) {
      using TI = decltype(ti);
      hipLaunchKernelGGL(beats_patch_kernel<TI>, grid, block, 0, st, (const TI*)fbank, big, total8, frames, P, c.mel_bins, c.patch);
    });
    GemmProb p{};
    p.A = big; p.a = plain((int)M, kp); p.W = h->wpatch; p.C = x; p.c = plain((int)M, Em);
    p.M = (int)M; p.N = Em; p.K = kp;
    if ((rc = launch_gemm(&p, 1, EPI_F32, OP_F16, st))) return chk(rc, "beats patch gemm");
    if ((rc = ln_rows(x, M, Em, h->lnpg, h->lnpb, c.ln_eps, 1.f, nullptr, a16, st))) return chk(rc, "beats patch layer norm");
    GemmProb q{};
    q.A = a16; q.a = plain((int)M, Em); q.W = h->wproj; q.bias = h->bproj; q.C = x; q.c = plain((int)M, D);
    q.M = (int)M; q.N = D; q.K = Em;
    if ((rc = launch_gemm(&q, 1, EPI_F32, OP_F16, st))) return chk(rc, "beats projection gemm");
  }
  if ((rc = beats_posconv(h, x, n, P, st))) return rc;
  const float alpha = c.deep_norm_alpha;
  if ((rc = ln_rows(x, M, D, h->lneg, h->lneb, c.ln_eps, alpha, x, a16, st))) return chk(rc, "beats encoder layer norm");
  for (int li = 0; li < c.layers; ++li) {
    const BeatsLayer& L = h->layers[li];
    const bool last = li + 1 == c.layers;
    {
      GemmProb p{};
      p.A = a16; p.a = plain((int)M, D); p.W = L.wqkv; p.bias = L.bqkv; p.C = big; p.c = plain((int)M, 3 * D);
      p.M = (int)M; p.N = 3 * D; p.K = D; p.persist = h->gemm_persist;
      if ((rc = launch_gemm(&p, 1, EPI_OP, OP_F16, st))) return chk(rc, "beats qkv gemm");
    }
    if ((rc = beats_attention(h, L, big, a16, n, P, ctx, st))) return rc;
    auto residual_gemm = [&](const void* A, int K, const void* W, const float* bias) {
      GemmProb p{};
      p.A = A; p.a = plain((int)M, K); p.W = W; p.bias = bias;
      p.R = x; p.r = plain((int)M, D); p.C = x; p.c = plain((int)M, D);
      p.M = (int)M; p.N = D; p.K = K;
      return launch_gemm(&p, 1, EPI_RES_F32, OP_F16, st);   // x = alpha x_prev (the stream) + A W^T + b
    };
    if ((rc = residual_gemm(ctx, D, L.wout, L.bout))) return chk(rc, "beats out_proj gemm");
    if ((rc = ln_rows(x, M, D, L.ln1g, L.ln1b, c.ln_eps, alpha, x, a16, st))) return chk(rc, "beats self_attn_layer_norm");
    {
      GemmProb p{};
      p.A = a16; p.a = plain((int)M, D); p.W = L.wfc1; p.bias = L.bfc1; p.C = big; p.c = plain((int)M, I);
      p.M = (int)M; p.N = I; p.K = D; p.persist = h->gemm_persist;
      if ((rc = launch_gemm(&p, 1, EPI_GELU_OP, OP_F16, st))) return chk(rc, "beats fc1 gemm");
    }
    if ((rc = residual_gemm(big, I, L.wfc2, L.bfc2))) return chk(rc, "beats fc2 gemm");
    if ((rc = ln_rows(x, M, D, L.ln2g, L.ln2b, c.ln_eps, last ? 1.f : alpha, x, last ? nullptr : a16, st))) return chk(rc, "beats final_layer_norm");
  }
  return hipGetLastError() == hipSuccess ? MRA_OK : fail(MRA_EHIP, "beats forward launch");
}

int mra_debug_beats_attention(mra_beats* h, int32_t layer, const void* qkv, const void* gate_src, int32_t n, int32_t tokens, void* ctx, void* stream_) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  const mra_beats_cfg& c = h->cfg;
  if (n < 0) return fail(MRA_EINVAL, "negative chunk count");
  if (layer < 0 || layer >= c.layers) return fail(MRA_EINVAL, "layer out of range");
  if (tokens <= 0 || tokens > MAX_TOKENS) return fail(MRA_EINVAL, "tokens per chunk must be in [1, 512]");
  if (n == 0) return MRA_OK;
  if (!qkv || !ctx || (c.gate_from == MRA_BEATS_GATE_INPUT && !gate_src)) return fail(MRA_EINVAL, "null argument");
  const std::string p = "encoder.layers." + std::to_string(layer) + ".self_attn.";
  if (!beats_loaded(h, {"encoder.layers.0.self_attn.relative_attention_bias.weight", p + "grep_linear.weight", p + "grep_linear.bias", p + "grep_a"}))
    return fail(MRA_ESTATE, "the bias table or the layer's gate parameters are not loaded");
  if ((long long)n * tokens * 3 * c.dim > 0x7fffffffLL) return fail(MRA_EINVAL, "too many chunks for one call: split them");
  const int rc = beats_attention(h, h->layers[layer], (const f16*)qkv, (const f16*)gate_src, n, tokens, (f16*)ctx, as_stream(stream_));
  if (rc) return rc;
  return hipGetLastError() == hipSuccess ? MRA_OK : fail(MRA_EHIP, "beats attention launch");
}

int mra_debug_beats_posconv(mra_beats* h, float* x, int32_t n, int32_t tokens, void* stream_) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (n < 0) return fail(MRA_EINVAL, "negative chunk count");
  if (tokens <= 0 || tokens > MAX_TOKENS) return fail(MRA_EINVAL, "tokens per chunk must be in [1, 512]");
  if (n == 0) return MRA_OK;
  if (!x) return fail(MRA_EINVAL, "null argument");
  if (!beats_loaded(h, {"encoder.pos_conv.0.weight", "encoder.pos_conv.0.bias"})) return fail(MRA_ESTATE, "encoder.pos_conv.0.* is not loaded");
  if ((long long)n * tokens * h->cfg.dim > 0x7fffffffLL) return fail(MRA_EINVAL, "too many chunks for one call: split them");
  const int rc = beats_posconv(h, x, n, tokens, as_stream(stream_));
  if (rc) return rc;
  return hipGetLastError() == hipSuccess ? MRA_OK : fail(MRA_EHIP, "beats posconv launch");
}

double mra_beats_flops(mra_beats* h, int32_t n, int32_t frames) {
  if (!h) return 0.0;
  const mra_beats_cfg& c = h->cfg;
  const double p = beats_tokens(c, frames), d = c.dim, I = c.ffn;
  const double layer = 2 * p * d * 3 * d + 4 * p * p * d + 2 * p * d * d + 4 * p * d * I;
  const double front = 2 * p * c.patch * c.patch * c.embed_dim + 2 * p * c.embed_dim * d;
  const double conv = 2 * p * d * (d / c.conv_pos_groups) * c.conv_pos;
  return n * (c.layers * layer + front + conv);
}

}  // extern "C"
