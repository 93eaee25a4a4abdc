// One whole token of the attached LM's greedy decode: replaces everything around the one-token attention inside the reference's
// self.llm_model.generate(inputs_embeds=..., attention_mask=..., max_new_tokens=64) (models/xinstructblip.py:383-391, utils/trainer.py:157-165):
// RMSNorm, the seven linears of a Llama layer, rotary, the cache write, SwiGLU, the residuals, the head and the greedy bookkeeping.
//   lm_embed_kernel    h[b] = table[tokens[b]]                                       a token outside [0, V) gives a row of NaN, nothing is read
//   lm_prep_kernel     xn[b] = (x[b] * rsqrt(mean(x[b]^2) + eps)) * gain  (fp32)     and u[a][b] = A_a xn[b] (fp32 [B][R]) for up to three adapters
//   lm_skinny_kernel   y[b][n] = sum_k x[b][k] W[n][k], 1 <= B <= 8, W read as stored ([N][K], pitch ldw): a wave owns LM_CPW columns at a time and
//                      streams their rows straight to registers with 16-byte loads; every lane keeps B x LM_CPW fp32 accumulators over its K chunks
//                      (k ascending, packed fp32 FMA over column pairs), a fixed xor tree adds the lanes.  Up to three (W, N) segments share x.  Epilogues (fp32 until the one store):
//                      plain | + residual | SwiGLU (the block streams gate AND up of its columns) | rotary + cache write (the block owns a head)
//   lm_argmax_kernel   first maximum of the fp32 logits (a NaN counts as the maximum, as torch.argmax: the first NaN wins) + generate's greedy
//                      bookkeeping: a finished sequence emits pad, a sequence that emits an eos id becomes finished
// No atomics, no inline assembly, no wait between workgroups: a seam between stages is a launch boundary.  Two runs give the same bits.
#include "kernels.h"
#include "mra_common.h"

namespace mra {
namespace {

constexpr int LM_CPW = 4;   // columns per wave and pass

__device__ __forceinline__ float block_sum256(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// grid B, 64 threads
template <typename T>
__global__ __launch_bounds__(64) void lm_embed_kernel(const int* __restrict__ tokens, const T* __restrict__ table, long long ld, int V, int K,
                                                      T* __restrict__ h, long long ldh) {
  const int b = blockIdx.x, tok = tokens[b];
  const bool ok = tok >= 0 && tok < V;
  typedef typename Vec8<T>::type V8;
  V8 nan8;
#pragma unroll
  for (int e = 0; e < 8; ++e) nan8[e] = from_f32<T>(__builtin_nanf(""));
  for (int c = threadIdx.x; c < K / 8; c += 64)
    *reinterpret_cast<V8*>(h + (long long)b * ldh + c * 8) = ok ? *reinterpret_cast<const V8*>(table + (long long)tok * ld + c * 8) : nan8;
}

// grid B, 256 threads
template <typename T>
__global__ __launch_bounds__(256) void lm_prep_kernel(LmPrep p) {
  __shared__ float red[4];
  typedef typename Vec8<T>::type V8;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, K8 = p.K / 8;
  const T* xr = (const T*)p.x + (long long)b * p.ldx;
  const T* g = (const T*)p.gain;
  float rs = 1.f;
  if (g) {
    float ss = 0.f;
    for (int c = tid; c < K8; c += 256) {
      const V8 x = *reinterpret_cast<const V8*>(xr + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss = fmaf((float)x[e], (float)x[e], ss);
    }
    ss = block_sum256(ss, red);
    rs = rsqrtf(ss / (float)p.K + p.eps);
    for (int c = tid; c < K8; c += 256) {
      const V8 x = *reinterpret_cast<const V8*>(xr + c * 8);
      const V8 gg = *reinterpret_cast<const V8*>(g + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) p.xn[(long long)b * p.K + c * 8 + e] = ((float)x[e] * rs) * (float)gg[e];
    }
  }
  // u[a][b][j] = sum_k A_a[j][k] xn[b][k]: a wave owns a (adapter, j) pair at a time
  const int total = p.R[0] + p.R[1] + p.R[2];
  for (int pj = wave; pj < total; pj += 4) {
    int a = 0, j = pj;
    if (j >= p.R[0]) { j -= p.R[0]; a = 1; }
    if (a == 1 && j >= p.R[1]) { j -= p.R[1]; a = 2; }
    const float* A = a == 0 ? p.A[0] : a == 1 ? p.A[1] : p.A[2];
    float* u = a == 0 ? p.u[0] : a == 1 ? p.u[1] : p.u[2];
    const int R = a == 0 ? p.R[0] : a == 1 ? p.R[1] : p.R[2];
    const float* Ar = A + (long long)j * p.K;
    float acc = 0.f;
    for (int c = lane; c < K8; c += 64) {
      const V8 x = *reinterpret_cast<const V8*>(xr + c * 8);
      V8 gg;
      if (g) gg = *reinterpret_cast<const V8*>(g + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = g ? ((float)x[e] * rs) * (float)gg[e] : (float)x[e];
        acc = fmaf(v, Ar[c * 8 + e], acc);
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) u[b * R + j] = acc;
  }
}

template <typename T, bool XF32>
__device__ __forceinline__ void load_x8(const void* x, long long off, float (&xf)[8]) {
  if constexpr (XF32) {
    const f32x4 a = *reinterpret_cast<const f32x4*>((const float*)x + off), c = *reinterpret_cast<const f32x4*>((const float*)x + off + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { xf[e] = a[e]; xf[4 + e] = c[e]; }
  } else {
    const typename Vec8<T>::type v = *reinterpret_cast<const typename Vec8<T>::type*>((const T*)x + off);
#pragma unroll
    for (int e = 0; e < 8; ++e) xf[e] = (float)v[e];
  }
}

// grid = the column blocks of every segment (SwiGLU: of one), 256 threads.  ys holds the block's fp32 products [matrix][row][column].
template <typename T, int BP, bool XF32>
__global__ __launch_bounds__(256) void lm_skinny_kernel(LmSkinny p) {
  __shared__ float ys[2][8][LM_MAX_CB];
  typedef typename Vec8<T>::type V8;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cb = p.cb, K8 = p.K / 8;
  int blk = blockIdx.x, s = 0;
  if (p.epi != LM_EPI_SWIGLU) {
    if (p.nseg > 1 && blk >= p.nblk[0]) { blk -= p.nblk[0]; s = 1; }
    if (s == 1 && p.nseg > 2 && blk >= p.nblk[1]) { blk -= p.nblk[1]; s = 2; }
  }
  const int n0 = blk * cb;
  const int nmat = p.epi == LM_EPI_SWIGLU ? 2 : 1;
  for (int mat = 0; mat < nmat; ++mat) {
    const int si = p.epi == LM_EPI_SWIGLU ? mat : s;
    LmSeg sg = p.seg[0];
    if (si == 1) sg = p.seg[1];
    if (si == 2) sg = p.seg[2];
    const T* W = (const T*)sg.W;
    for (int c0 = wave * LM_CPW; c0 < cb; c0 += 4 * LM_CPW) {
      if (n0 + c0 >= sg.N) break;                        // wave-uniform: nothing of this pass is inside the segment
      const T* wr[LM_CPW];
#pragma unroll
      for (int i = 0; i < LM_CPW; ++i) {
        const int n = n0 + c0 + i < sg.N ? n0 + c0 + i : sg.N - 1;      // the ragged tail reads the last row again and is dropped below
        wr[i] = W + (long long)n * sg.ldw;
      }
      f32x2 acc[LM_CPW / 2][BP];                       // column pairs: one packed fp32 fma serves two columns
#pragma unroll
      for (int i = 0; i < LM_CPW / 2; ++i)
#pragma unroll
        for (int b = 0; b < BP; ++b) acc[i][b] = f32x2{0.f, 0.f};
#pragma unroll 2
      for (int c = lane; c < K8; c += 64) {
        V8 w[LM_CPW];
#pragma unroll
        for (int i = 0; i < LM_CPW; ++i) w[i] = __builtin_nontemporal_load(reinterpret_cast<const V8*>(wr[i] + c * 8));
        f32x2 wf[LM_CPW / 2][8];
#pragma unroll
        for (int i = 0; i < LM_CPW / 2; ++i)
#pragma unroll
          for (int e = 0; e < 8; ++e) wf[i][e] = f32x2{(float)w[2 * i][e], (float)w[2 * i + 1][e]};
#pragma unroll
        for (int b = 0; b < BP; ++b) {
          if (b < p.B) {
            float xf[8];
            load_x8<T, XF32>(p.x, (long long)b * p.ldx + c * 8, xf);
#pragma unroll
            for (int i = 0; i < LM_CPW / 2; ++i)
#pragma unroll
              for (int e = 0; e < 8; ++e) acc[i][b] = __builtin_elementwise_fma(wf[i][e], f32x2{xf[e], xf[e]}, acc[i][b]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < LM_CPW; ++i)
#pragma unroll
        for (int b = 0; b < BP; ++b) {
          const float t = wave_sum(acc[i / 2][b][i % 2]);
          if (lane == 0) ys[mat][b][c0 + i] = t;
        }
    }
  }
  __syncthreads();
  // the LoRA term, on the products in fp32: t = sum_j u[b][j] Bw[n][j] (fma chain from 0, j ascending), y = fma(scale, t, y)
  for (int mat = 0; mat < nmat; ++mat) {
    const int si = p.epi == LM_EPI_SWIGLU ? mat : s;
    LmSeg sg = p.seg[0];
    if (si == 1) sg = p.seg[1];
    if (si == 2) sg = p.seg[2];
    if (sg.R > 0)
      for (int idx = tid; idx < p.B * cb; idx += 256) {
        const int b = idx / cb, c = idx % cb, n = n0 + c;
        if (n < sg.N) {
          float t = 0.f;
          for (int j = 0; j < sg.R; ++j) t = fmaf(sg.u[b * sg.R + j], sg.Bw[(long long)n * sg.R + j], t);
          ys[mat][b][c] = fmaf(sg.scale, t, ys[mat][b][c]);
        }
      }
  }
  __syncthreads();
  LmSeg sg = p.seg[0];
  if (s == 1) sg = p.seg[1];
  if (s == 2) sg = p.seg[2];
  for (int idx = tid; idx < p.B * cb; idx += 256) {
    const int b = idx / cb, c = idx % cb, n = n0 + c;
    if (n >= sg.N) continue;
    const float y = ys[0][b][c];
    if (p.epi == LM_EPI_PLAIN) {
      if (p.out_f32) ((float*)sg.out)[(long long)b * sg.ldo + n] = y;
      else ((T*)sg.out)[(long long)b * sg.ldo + n] = from_f32<T>(y);
    } else if (p.epi == LM_EPI_RES) {
      const float r = (float)((const T*)p.res)[(long long)b * p.ldres + n];
      ((T*)sg.out)[(long long)b * sg.ldo + n] = from_f32<T>(y + r);
    } else if (p.epi == LM_EPI_SWIGLU) {
      const float up = ys[1][b][c];
      ((T*)sg.out)[(long long)b * sg.ldo + n] = from_f32<T>((y / (1.f + expf(-y))) * up);
    } else {   // LM_EPI_ROPE: cb == D, the block is head blk of q (s 0), k (s 1) or v (s 2)
      float r = y;
      if (s < 2) {
        const long long pos = (long long)p.position[b] + p.pos_offset;
        if (pos < 0 || pos >= p.rope_rows) {
          r = __builtin_nanf("");                       // a position outside the table reads nothing
        } else {
          const int half = cb / 2;
          const float o = c < half ? -ys[0][b][c + half] : ys[0][b][c - half];
          r = fmaf(o, p.sin[pos * p.rope_ld + c], y * p.cos[pos * p.rope_ld + c]);
        }
      }
      if (s == 0) ((T*)sg.out)[(long long)b * sg.ldo + n] = from_f32<T>(r);
      else if (s == 1) ((T*)p.kc)[(long long)b * p.k_sb + (long long)blk * p.k_sh + (long long)p.slot * p.k_ss + c] = from_f32<T>(r);
      else ((T*)p.vc)[(long long)b * p.v_sb + (long long)blk * p.v_sh + (long long)p.slot * p.v_ss + c] = from_f32<T>(r);
    }
  }
}

// grid B, 256 threads.  (value, index) order: a NaN is above everything, then the larger value, then the LOWER index.
__device__ __forceinline__ bool lm_better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (!vn && v != bv) return v > bv;
  return i < bi;
}
__global__ __launch_bounds__(256) void lm_argmax_kernel(const float* __restrict__ logits, long long ld, int V, LmGreedy g) {
  __shared__ float sv[256];
  __shared__ int si[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* z = logits + (long long)b * ld;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid; i < V; i += 256)
    if (lm_better(z[i], i, bv, bi)) { bv = z[i]; bi = i; }
  sv[tid] = bv;
  si[tid] = bi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o && lm_better(sv[tid + o], si[tid + o], sv[tid], si[tid])) { sv[tid] = sv[tid + o]; si[tid] = si[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    int tok = si[0];
    if (g.finished) {
      if (g.finished[b]) tok = g.pad;
      bool stop = false;
      for (int e = 0; e < g.n_eos; ++e) stop = stop || tok == g.eos[e];
      if (stop) g.finished[b] = 1;
    }
    g.tokens_out[b] = tok;
  }
}

int last() { return hipGetLastError() == hipSuccess ? 0 : -4; }

template <typename T>
int skinny_typed(const LmSkinny& p, int grid, hipStream_t stream) {
  const int bp = p.B <= 1 ? 1 : p.B <= 2 ? 2 : p.B <= 4 ? 4 : 8;
#define MRA_LM_CASE(BPV)                                                                                           \
  case BPV:                                                                                                        \
    if (p.x_f32) hipLaunchKernelGGL((lm_skinny_kernel<T, BPV, true>), dim3(grid), dim3(256), 0, stream, p);        \
    else hipLaunchKernelGGL((lm_skinny_kernel<T, BPV, false>), dim3(grid), dim3(256), 0, stream, p);               \
    break;
  switch (bp) {
    MRA_LM_CASE(1)
    MRA_LM_CASE(2)
    MRA_LM_CASE(4)
    MRA_LM_CASE(8)
  }
#undef MRA_LM_CASE
  return last();
}

}  // namespace

int launch_lm_embed(const int* tokens, const void* table, long long ld, int V, int B, int K, void* h, long long ldh, int op_dtype,
                    hipStream_t stream) {
  if (B < 1 || B > LM_MAX_B || K < 8 || K % 8 || V < 1) return -1;
  if (op_dtype == OP_BF16) hipLaunchKernelGGL((lm_embed_kernel<bf16>), dim3(B), dim3(64), 0, stream, tokens, (const bf16*)table, ld, V, K, (bf16*)h, ldh);
  else hipLaunchKernelGGL((lm_embed_kernel<f16>), dim3(B), dim3(64), 0, stream, tokens, (const f16*)table, ld, V, K, (f16*)h, ldh);
  return last();
}

int launch_lm_prep(const LmPrep& p, int op_dtype, hipStream_t stream) {
  if (p.B < 1 || p.B > LM_MAX_B || p.K < 8 || p.K % 8) return -1;
  for (int a = 0; a < 3; ++a)
    if (p.R[a] < 0 || p.R[a] > LM_MAX_R) return -1;
  if (!p.gain && p.R[0] + p.R[1] + p.R[2] == 0) return 0;
  if (op_dtype == OP_BF16) hipLaunchKernelGGL((lm_prep_kernel<bf16>), dim3(p.B), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((lm_prep_kernel<f16>), dim3(p.B), dim3(256), 0, stream, p);
  return last();
}

int launch_lm_skinny(const LmSkinny& in, int op_dtype, hipStream_t stream) {
  LmSkinny p = in;
  if (p.B < 1 || p.B > LM_MAX_B || p.K < 8 || p.K % 8 || p.nseg < 1 || p.nseg > 3) return -1;
  if (p.epi == LM_EPI_ROPE) {
    if (p.nseg != 3 || (p.D != 64 && p.D != 128) || p.seg[0].N != p.Hq * p.D || p.seg[1].N != p.Hkv * p.D || p.seg[2].N != p.Hkv * p.D) return -1;
    p.cb = p.D;
  } else {
    if (p.epi == LM_EPI_SWIGLU && (p.nseg != 2 || p.seg[0].N != p.seg[1].N)) return -1;
    p.cb = LM_CB;
  }
  int grid = 0;
  for (int s = 0; s < 3; ++s) {
    p.nblk[s] = s < p.nseg ? (p.seg[s].N + p.cb - 1) / p.cb : 0;
    if (s < p.nseg && (p.seg[s].N < 1 || p.seg[s].R < 0 || p.seg[s].R > LM_MAX_R)) return -1;
    if (p.epi != LM_EPI_SWIGLU || s == 0) grid += p.nblk[s];
  }
  return op_dtype == OP_BF16 ? skinny_typed<bf16>(p, grid, stream) : skinny_typed<f16>(p, grid, stream);
}

int launch_lm_argmax(const float* logits, long long ld, int B, int V, const LmGreedy& g, hipStream_t stream) {
  if (B < 1 || V < 1 || g.n_eos < 0 || g.n_eos > LM_MAX_EOS) return -1;
  hipLaunchKernelGGL(lm_argmax_kernel, dim3(B), dim3(256), 0, stream, logits, ld, V, g);
  return last();
}

}  // namespace mra
