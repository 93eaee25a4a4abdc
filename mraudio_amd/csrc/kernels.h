// Host-visible launchers of the gfx950 kernels.  Everything takes raw device pointers and a
// stream; nothing here allocates, synchronises or touches torch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mra {

enum OpDtype { OP_F16 = 0, OP_BF16 = 1 };

// GEMM epilogues (C index is [activation row m][weight row n])
enum GemmEpi {
  EPI_OP = 0,       // C(op dtype) = acc + bias
  EPI_GELU_OP = 1,  // C(op dtype) = gelu_erf(acc + bias)
  EPI_RES_F32 = 2,  // C(f32)      = acc + bias + R
  EPI_F32 = 3,      // C(f32)      = acc + bias
  EPI_KV = 4,       // C(op dtype) head-major K/V cache, see GemmProb::kv_*
  EPI_GELU_BOTH = 6, // training forward: aux(op dtype) = acc + bias (the pre-activation the backward needs), C(op dtype) = gelu_erf of it
  EPI_GELU_BWD = 7,  // training backward: C(op dtype) = acc * gelu'(aux): the GELU gradient inside the data-gradient GEMM
  EPI_RES_OP = 8,   // C(op dtype) = op(acc + bias) + Rop: residual stream kept in the operand dtype (the ViT under precision="fp16");
                    // Rop is GemmProb::aux (op dtype, addressed like C; may alias C: updated in place)
  EPI_RES_LN = 9,   // EPI_RES_F32 followed by the LayerNorm of the finished rows INSIDE the launch (ring tiles only): the column tile of a row block
                    // that finishes last (agent-scope counter GemmProb::ln_counter, one per row tile, zero before the launch, reset by the kernel)
                    // normalises the block's rows and writes ln_y32 / ln_y16 -- the reference's `LayerNorm(dense(x) + residual)` (HF:519-530,
                    // 573-587) in one launch.  C still receives the pre-LayerNorm rows (sc1 stores: other XCDs read them).
  // LayerNorm folded into the GEMMs on either side of it (the ViT blocks, fp32 residual stream): y = LN(x) W^T + b with LN's gain inside
  // W' = W diag(g) is  rstd[m] * (x W'^T - mu[m] * colsum(W')[n]) + (b + W beta)[n]  -- a GEMM over the op-dtype copy of the RAW rows x plus a
  // rank-one correction in the epilogue.  The producer of x (a residual GEMM) emits that copy and the row statistics as it stores x:
  EPI_RES_F32_STAT = 10,  // EPI_RES_F32, plus: ln_y16 (op dtype, row view ln_y16v) = the finished rows, and per (row, 128-column group) the
                          // group mean and the group's sum of squared deviations, ln_y32[(m * (N / 128) + n / 128) * 2 + {0, 1}]
                          // (launch_ln_group_stats folds the groups into (mean, rstd) per row).  Eight-phase tiles only (a wave owns 128 columns).
  EPI_RES_OP_STAT = 13,   // EPI_RES_OP (residual stream in the operand dtype), plus the statistics of the ROUNDED rows per (row, 64-column block):
                          // ln_y32[(m * (N / 64) + n / 64) * 2 + {0, 1}]; the stream itself is the consumer's operand, no copy.  Eight-phase tiles only.
  EPI_LNF_OP = 11,        // C(op dtype) = rstd[m] * (acc - mu[m] * ln_gain[n]) + bias[n]; (mu, rstd)[m] = ln_y32[2 m], ln_y32[2 m + 1]; ln_gain = colsum(W')
  EPI_LNF_GELU_OP = 12,   // gelu_erf of the same (256 x 256 eight-phase tile only, both)
  EPI_SOFTPART = 5, // C(op dtype) = exp2(alpha * acc - max over the tile's columns of the row); the row's tile maximum and tile
                    // sum go to stat_m / stat_l [row][ntiles] (176 x 384 loader-wave tile only: a wave holds whole tile rows)
};

// Tile configurations of launch_gemm (GemmProb::tile_cfg), weight rows x activation rows.  The numbers are recorded in profiles and DESIGN tables.
enum GemmTile {
  GT_AUTO = 0,          // the largest of 64 / 128 / 256 that divides N (or n_ragged / n_mask) and still fills the CUs
  GT_64 = 1,            // 64 x 64 two-buffer loop; 128-deep K steps from K >= 2048 (K % 128 == 0)
  GT_128 = 2,           // 128 x 128 two-buffer loop
  GT_256 = 3,           // 256 x 256: eight-phase kernel when every problem has an even number of K steps, else the loader-wave kernel
  GT_WS_128x384 = 4,    // loader-wave tile of the folded cross-attention (EPI_OP / EPI_F32; w_kwrap)
  GT_WS_176x384 = 5,    // loader-wave tile with the compute waves in one column (N % 176 == 0 unless n_ragged; w_ld, w_kwrap, pscale, EPI_SOFTPART)
  GT_K128_64x128 = 6,   // 128-deep K steps (K % 128 == 0): the long-K down-projections of the layer chain at ~1 k rows
  GT_P8_TAIL = 7,       // eight-phase 128 x 512, N = 128 exactly: the half-width last column tile of N = 256 k + 128 as a launch of its own (W / bias / C / R offset to those columns)
  GT_P8_MIXED = 8,      // N = 256 k + 128 in ONE launch: full 256 x 256 eight-phase tiles + one 128 x 512 tail tile per pair of row tiles (one problem)
  GT_RING_144x128 = 9,  // the ring kernel's exact-fit tiles of the layer chain (plain problems, N a multiple of the tile): QKV 2048 x 2304,
  GT_RING_192x128 = 10, // FFN-up 2 x 1024 x 3072,
  GT_RING_96x64 = 11,   // the N = 768 projections (the only tile with EPI_RES_LN)
  GEMM_TILES = 12
};

// Logical activation row m of a "row view" lives at base + (m / rpi) * item_stride + (m % rpi) * ld
// (elements).  This lets the 32 query rows or the L text rows of every [S, H] item be addressed in
// place, without gathers.
struct RowView {
  long long item_stride;
  int rpi;  // rows per item
  int ld;   // row stride
};

// One problem of a (possibly grouped) launch: C[m][n] = sum_k A[m][k] * W[n][k] (+ epilogue).
struct GemmProb {
  const void* A;      // activations, op dtype, row view `a`
  const void* W;      // weights [N][K] row-major (the reference's nn.Linear layout), op dtype
  const float* bias;  // [N] or nullptr
  void* C;            // row view `c`
  const float* R;     // residual (EPI_RES_F32), row view `r`
  void* aux;          // EPI_GELU_BOTH (written) / EPI_GELU_BWD (read): op-dtype tensor addressed like C (row view `c`)
  RowView a, c, r;
  int M, N, K;
  // EPI_KV: weight row n = (cl * 2 + kv) * hidden + head * 64 + d ; activation row m = item * kv_tokens + tok
  // destination element ((((cl * 2 + kv) * kv_items + item) * kv_heads + head) * kv_tokens + tok) * 64 + d
  int kv_tokens, kv_items, kv_heads;
  // Batched launch (batch > 1): problem b uses A + b * a_bs, W + b * w_bs (elements), bias + b * bias_bs and
  // C + b * c_bs_bytes; M, N, K and the row views are shared.  Tiles never straddle batch entries.
  int batch;
  long long a_bs, w_bs, c_bs_bytes;
  int bias_bs;
  // n_ragged: N need not be a multiple of the tile; weight rows past N - 1 are read from row N - 1 and their
  // output columns are written anyway, so C rows must hold ceil(N / tile) * tile columns and bias must be null.
  int n_ragged;
  // n_mask (EPI_RES_F32 / EPI_F32): N need not be a multiple of the tile either, but output columns past N - 1 are simply not
  // stored (bias and residual are not read there): C keeps its plain [M][N] rows.  N % 4 == 0.
  int n_mask;
  // w_ld > 0 (176 x 384 loader-wave tile, EPI_OP only): W is given K-major, W[k][n] at W + k * w_ld + n (a plain [K][N] row-major
  // matrix, e.g. the encoder tokens themselves for P . enc); rows k >= k_rows are read from row k_rows - 1 (the A operand
  // is zero there).  The kernel stages [64 k][176 n] tiles and takes its fragments with ds_read_b64_tr_b16.
  int w_ld, k_rows;
  // EPI_RES_LN: LayerNorm over the N columns of every finished row (N = 256 k <= 1024): y = (x - mean) * rstd * ln_gain + ln_bias, biased variance,
  // fp32; outputs ln_y32 (fp32, row view ln_y32v; may be null) and ln_y16 (operand dtype, row view ln_y16v; may be null)
  const float* ln_gain;
  const float* ln_bias;
  float ln_eps;
  float* ln_y32;
  void* ln_y16;
  RowView ln_y32v, ln_y16v;
  unsigned* ln_counter;   // [ceil(M / tile rows)] zero before the launch; the kernel leaves it zero
  // w_kwrap > 0 (loader-wave kernels, row-major W): W holds only w_kwrap K steps of 64 (K = 2 * 64 * w_kwrap) and is walked twice -- C = [A_hi | A_lo] . [W | W]^T,
  // the scores product of the split-precision cross-attention (Q' kept as an f16 hi + lo pair against the same encoder slab)
  int w_kwrap;
  // EPI_SOFTPART: scale of the scores in log2 units and the per-(row, column tile) statistics, row m of batch entry b at
  // stat_*[(b * M + m) * ntiles + tile]
  float alpha;
  float* stat_m;
  float* stat_l;
  // pscale != nullptr (176 x 384 loader-wave tile with K-major W only): the A operand is the unnormalised P~ of the split softmax; A[m][k]
  // is multiplied by pscale[((batch entry * ps_ntiles) + min(k / 176, ps_ntiles - 1)) * 512 + m] on its way into the MFMA (f16: packed
  // multiplies with the factor rounded to f16; bf16: in fp32, rounded once -- what the separate rescale pass did in HBM).  A must be
  // ZERO from column ps_ntiles * 176 on (launch_fold_rowfactor does that).  M <= 384 (one row tile: the kernel indexes the
  // 512-row factor slice by the row inside the tile).
  const float* pscale;
  int ps_ntiles;
  // col_scale != nullptr (EPI_SOFTPART with row-major W only): the weight-side rows are RAW tokens whose LayerNorm is folded into the other
  // operand; column n of batch entry b carries the factor r = col_scale[b * cs_bs + n] (1 / sqrt(var + eps) of token n).  The epilogue takes
  // the tile maximum over r * acc, writes C = T(exp2(alpha * r * acc - stat_m) * r) and keeps stat_l the fp32 sum of the exponentials
  // themselves (without r, before any rounding to T).
  // col_stats != 0: the kernel computes the factors itself from the weight-side rows as they pass through LDS (biased variance over K,
  // cs_eps) and WRITES col_scale[b * cs_bs + n] for n < N (no w_kwrap: one pass over the rows); otherwise col_scale is read.
  float* col_scale;
  long long cs_bs;
  int col_stats;
  float cs_eps;
  int tile_cfg;    // a GemmTile; in a grouped launch the first problem decides
  int order;       // tile walk: 0 = panels of 8 row tiles, rows fastest; gn > 0 = panels of gn column tiles walked down the rows, columns
                   // fastest (measured better for the ViT's N = 1408 GEMMs: all 6 column tiles of a row tile run together)
  int persist;     // eight-phase 256 x 256 kernel, staged epilogues: 1 = ONE workgroup per CU walks over the tiles (blockIdx, + gridDim, ...) instead of one
                   // workgroup per tile.  A stamped timeline (gemm_bench p8stamp, fc1 shape) shows ~3.8 us between the end of a workgroup and the start
                   // of the next on its CU plus ~1.8 us of kernel entry / argument fetch / address set-up per workgroup, of a ~50 us tile
  int tile_begin;  // filled by the launcher
  int mtiles, ntiles;
  int batch_row0;  // filled per workgroup: first row of its batch entry in the EPI_SOFTPART statistics
  int k128;        // GT_64 only: 128-deep K steps (gemm_k128_kernel's 64 x 64 tile) whenever K % 128 == 0, not only from K = 2048 on -- the folded
                   // context GEMM at K = enc_width (mra_qformer_set_option "cross_fuse" bit 4); same ascending K order, same bits
  int ps_stats;    // 1 (176 x 384 loader-wave tile with K-major W, instead of pscale): the row factors are computed in the launch from the tile
                   // statistics stat_m / stat_l [batch * M][ps_ntiles] of the scores launch (fold_rowfactor_kernel's arithmetic and reduction
                   // order: the same bits), and A need NOT be zero from column ps_ntiles * 176 on -- those columns are zeroed in LDS
};

constexpr int GEMM_MAX_GROUPS = 4;   // problems per launch (round 3: the pair forward groups the query / text problems of two Q-Formers)
struct GemmArgs {
  GemmProb p[GEMM_MAX_GROUPS];
  int ngroups;
  int total_tiles;
  unsigned long long* dbg;  // diagnostic builds only (gemm_set_debug_buffer): per-wave cycle sums
  int order;                // 0: 8-row-tile panels, rows fastest; gn > 0: panels of gn column tiles, columns fastest (GemmProb::order of the first problem)
};

// Returns 0 on success, <0 on bad shapes.  All problems of one launch share dtype / epilogue.
int launch_gemm(const GemmProb* probs, int ngroups, int epi, int op_dtype, hipStream_t stream);
// Everything launch_gemm decides short of launching.  gemm_plan is host-only and makes no HIP call: validates the problems, picks the tile and
// the kernel family, and fills the kernel argument.  Returns 0, -1 (bad problem) or -2 (the tile has no such epilogue); launch_gemm adds
// -3 / -4 (runtime).
struct GemmPlan {
  int cus;          // in: CU count of the device; a persistent launch (GemmProb::persist) needs it, 0 = one workgroup per tile
  int tile;         // GemmTile, never GT_AUTO
  int family;       // GemmFamily
  int threads, lds; // block size, dynamic LDS bytes
  int persistent;   // 1: eight-phase 256 x 256 kernel as `grid` = cus & ~7 workgroups that walk over the tiles
  int grid;
  GemmArgs args;    // tile_begin / mtiles / ntiles of every problem, total_tiles, order
};
int gemm_plan(const GemmProb* probs, int ngroups, int epi, int op_dtype, GemmPlan* out);
// Main loops ("families") launch_gemm dispatches to, and a read-only launch counter per (family, epilogue) since the library was
// loaded (mra_debug_gemm_launches in include/mra.h): parity tests use it to state which kernel produced the numbers they checked.
enum GemmFamily {
  GF_V1_64 = 0, GF_V1_128 = 1, GF_V1_256 = 2,   // gemm_kernel two-buffer loop (256: experiment builds only, gemm_force_variant(1))
  GF_WS_256 = 3,                                // gemm_ws_kernel 256 x 256 (odd number of K steps)
  GF_P8_256 = 4,                                // gemm_p8_kernel eight-phase 256 x 256
  GF_WS_128x384 = 5, GF_WS_176x384 = 6,         // loader-wave tiles of the folded cross-attention
  GF_K128_64x128 = 7,                           // gemm_k128_kernel, 128-deep steps
  GF_P8_TAIL = 8, GF_P8_MIXED = 9,              // eight-phase 128 x 512 tail tile; full tiles + tail tile in one launch
  GF_K128_64x64 = 10,
  GF_RING_144x128 = 11, GF_RING_192x128 = 12, GF_RING_96x64 = 13,   // gemm_ring_kernel: exact-fit tiles of the layer chain, K tiles through an LDS ring
  GEMM_FAMILIES = 14
};
long long gemm_launch_count(int family, int epi);
#ifdef MRA_GEMM_EXPERIMENTS
// Process-global A/B switches: compiled ONLY into tests/native/libmra_hip_exp.so (the experiment library of tests/native/gemm_bench and
// kernel_check_exp); the shipped libmra_hip.so has no mutable global state besides the launch counters above.
void gemm_force_config(int tile); // a GemmTile for every later launch, over GemmProb::tile_cfg; GT_AUTO = off (default)
void gemm_set_debug_buffer(unsigned long long* dev_buf);  // variant 4 (stamped v1) writes 4 u64 per wave
void gemm_set_eight_phase(int on);         // 256 x 256 launches with an even number of K steps on gemm_p8_kernel (A/B switch)
void gemm_set_tile_order(int order);      // overrides GemmProb::order for every later launch when != 0 (A/B runs)
void gemm_force_variant(int v);   // 5 = default (warp-specialised 256x256, two-buffer small tiles); 0 ring, 1 two-buffer,
                                  // 2 +L2 prefetch, 3 +spread DMA issue, 4 stamped diagnostic -- kept for A/B runs
#endif

// ---- backward-pass GEMMs ------------------------------------------------------------------------
// dW[n][k] (+)= sum_m dY[m][n] * X[m][k].  dY and X are given as 64-column blocks: block b of dY starts at
// dY + b * y_block_stride and its row m at + row-view(yv, m) (row-major [M, N]: block stride 64, ld N;
// head-major K/V gradients: block = (layer, k|v, head), stride kv * 64, item stride heads * kv * 64, ld 64).
struct GemmTnArgs {
  const void* dY;
  const void* X;
  float* dW;   // [N][ldw] f32
  RowView yv, xv;
  long long y_block_stride, x_block_stride;
  int M, N, K;
  int ldw;
  int accumulate;  // 1: dW += ...
  float* db;       // optional bias gradient db[n] += sum_m dY[m][n], always accumulated (the column-block-0 workgroups
                   // multiply their dY fragments by a ones operand: two more MFMAs per step instead of a second launch)
};
int launch_gemm_tn(const GemmTnArgs& a, int op_dtype, hipStream_t stream);
// Up to GEMM_TN_MAX_JOBS weight gradients in ONE launch (the weight gradients that become computable at the same point of the backward:
// query / key / value / output of a self-attention, the two matrices of a feed-forward, ...).  A weight gradient of the layer chain is ~150
// output tiles of a few hundred contraction rows: a launch of its own is a chip full of short, latency-bound workgroups (21 us on average, 240
// of them per training step); launched together the jobs' workgroups share the CUs.  All jobs must be accumulating (dW += ...) when the
// contraction is split (it is split by the same factor for every job).
constexpr int GEMM_TN_MAX_JOBS = 4;
struct GemmTnGroup {
  GemmTnArgs j[GEMM_TN_MAX_JOBS];
  int njobs;
  int nb_begin[GEMM_TN_MAX_JOBS + 1];   // filled by the launcher: first 64-row block of dW (grid.x index) of every job
};
int launch_gemm_tn_group(const GemmTnArgs* jobs, int njobs, int op_dtype, hipStream_t stream);
// Encoder-side data gradient of the cross K / V projections (enc_grad.hip): d_enc [Ne * kv][E] fp32 = dKV W, with dKV the head-major dK / dV
// tape [nsel][Ne][heads][kv][64] (operand dtype, nsel = ncross * 2) read in place and W [nsel * heads * 64][E] as stored.  E % 128 == 0.
int launch_kvgrad_gemm(const void* dkv, const void* W, float* d_enc, int Ne, int kv, int heads, int nsel, int E, int op_dtype, hipStream_t stream);
// The same kernel on a plain row-major A (its second A-side addressing mode): dX [M][E] fp32 = dY W, dY [M][K] operand dtype with contiguous
// K (16-byte aligned rows), W [K][E] as stored -- the data gradient of a linear layer y = x W^T without a transposed copy of W.  K % 64 == 0,
// E % 128 == 0; dX is written, rows past M are loaded clamped and not stored; no atomics.
int launch_rowgrad_gemm(const void* dY, const void* W, float* dX, int M, int K, int E, int op_dtype, hipStream_t stream);
// Backward of the LLM projection y = op(z) W^T + b (proj_grad.hip), W [Lh][H] operand dtype: d_z [R][H] = dY W (written, one
// launch_rowgrad_gemm), d_W [Lh][H] += dY^T op(z) and d_b [Lh] += colsum(dY) (one launch_gemm_tn with its db output; d_b alone: the same
// launch on the first 64 columns of op(z) into `scratch` [Lh][64], so its bits are those of the joint call).  dY [R][Lh] operand dtype, z16 =
// op(z) [R][H]; every output may be NULL.  Lh % 64 == 0, H % 128 == 0.
int launch_llm_proj_bwd(const void* dY, const void* z16, const void* W, int R, int Lh, int H, float* d_z, float* d_W, float* d_b, float* scratch,
                        int op_dtype, hipStream_t stream);
// The low-rank branch of an adapted linear (lora.hip; R <= 16, widths and pitches multiples of 8 elements, 16-byte aligned rows).  A small fp32
// matrix over (width index n, rank index j) is stored [width][R] (LORA_NR, as lora_B) or [R][width] (LORA_RN, as lora_A).  thr = round(p 2^32) is
// the dropout threshold of keep(seed, m * width + n) (0: no mask, no hashing); the scale is the caller's (1/q, alpha / R, a loss scale divided out).
enum LoraLayout { LORA_NR = 0, LORA_RN = 1 };
// out [M][R] fp32 = scale * drop(X)[M][K] op(W)^T, X in the operand dtype with pitch ldx, W fp32 rounded on its way in.
int launch_lora_down(const void* X, long long ldx, int M, int K, const float* W, int R, int w_layout, float scale, unsigned thr,
                     unsigned long long seed, float* out, int op_dtype, hipStream_t stream);
// Y [M][N] (operand dtype, pitch ld) = op(float(Y) + scale * keep * U [M][R] W), in place; fp32 fma chain over j ascending.
int launch_lora_up_add(void* Y, long long ld, int M, int N, const float* U, int R, const float* W, int w_layout, float scale, unsigned thr,
                       unsigned long long seed, int op_dtype, hipStream_t stream);
// dW (fp32, either layout) += scale * drop(X)[M][N]^T op(U)[M][R]; a workgroup owns 32 columns and walks all rows, no atomics.
int launch_lora_wgrad(const void* X, long long ld, int M, int N, const float* U, int R, float* dW, int dw_layout, float scale, unsigned thr,
                      unsigned long long seed, int op_dtype, hipStream_t stream);
// The LM head + cross-entropy on gathered rows (lm_head.hip).  Geometry the workspace layout depends on: 64-column vocabulary tiles, 128-row
// groups, 128-column hidden blocks in the backward, whose contraction over V is split into at most 16 ranges of whole tiles (about 512
// workgroups on a large shape); lm_head_splits is the number of fp32 partial-sum planes [R][K] the backward writes and reduces in order.
constexpr int LM_HEAD_TILE = 64, LM_HEAD_ROWS = 128, LM_HEAD_KBLOCK = 128, LM_HEAD_MAX_SPLITS = 16;
inline int lm_head_tiles(int V) { return (V + LM_HEAD_TILE - 1) / LM_HEAD_TILE; }
inline int lm_head_splits(int R, int V, int K) {
  const long long wgs = (long long)((K + LM_HEAD_KBLOCK - 1) / LM_HEAD_KBLOCK) * ((R + LM_HEAD_ROWS - 1) / LM_HEAD_ROWS);
  long long smax = wgs > 0 ? 512 / wgs : 1;
  smax = smax < 1 ? 1 : (smax > LM_HEAD_MAX_SPLITS ? LM_HEAD_MAX_SPLITS : smax);
  const int nt = lm_head_tiles(V), tps = (int)((nt + smax - 1) / smax);
  return (nt + tps - 1) / tps;
}
// H [R][K], W [V][K] (operand dtype, pitches ldh / ldw), labels int32 [R] -> nll, lse f32 [R]; tmax, tsum f32 [R][tiles], zy f32 [R] and
// P (operand dtype [R][64 tiles], NULL: not written) are workspace.  One W pass + a merge launch.
int launch_lm_head_fwd(const void* H, long long ldh, int R, int K, const void* W, long long ldw, int V, const int* labels, float* nll, float* lse,
                       float* tmax, float* tsum, float* zy, void* P, int op_dtype, hipStream_t stream);
// dh [R][K] (operand dtype, pitch lddh) = sum_v g_r exp(tmax - lse) P~ W - g_r W[y_r]; part f32 [lm_head_splits][R][K] is workspace.
int launch_lm_head_bwd(const float* g, const void* W, long long ldw, int V, int K, const int* labels, const float* lse, const float* tmax,
                       const void* P, float* part, void* dh, long long lddh, int R, int op_dtype, hipStream_t stream);
// One-token attention over a K/V cache read in place (decode_attn.hip): q, out [B][Hq][D], k, v [B][Hkv][S][D] in the operand dtype with element
// strides (D contiguous, every stride a multiple of 8), mask [B][S] bytes (NULL: all attended), lse f32 [B][Hq] (may be NULL).  A workgroup owns
// DECODE_CHUNK keys of one (b, kv head) for all Hq / Hkv query heads; pm, pl f32 [B][Hq][chunks] and pacc f32 [B][Hq][chunks][D] are workspace.
// D in {64, 128}, Hq / Hkv in {1, 2, 4, 8}; two launches, no atomics.
constexpr int DECODE_CHUNK = 256;
inline int decode_chunks(int S) { return (int)(((long long)S + DECODE_CHUNK - 1) / DECODE_CHUNK); }
struct DecodeArgs {
  const void* q; long long q_sb, q_sh;
  const void* k; long long k_sb, k_sh, k_ss;
  const void* v; long long v_sb, v_sh, v_ss;
  const unsigned char* mask; long long mask_sb;
  int B, Hq, Hkv, S;
  float scale;
  void* out; long long o_sb, o_sh;
  float* lse;
  float *pm, *pl, *pacc;                        // workspace
};
int launch_decode_attention(const DecodeArgs& a, int D, int op_dtype, hipStream_t stream);
// Causal grouped-query attention of the LM's prefill (prefill_attn.hip): q [B][Hq][Sq][D], k, v [B][Hkv][Skv][D] in the operand dtype with
// element strides (D contiguous, every stride a multiple of 8), mask [B][Skv] bytes (NULL: all attended), query row i at key slot q_offset + i,
// out [B][Sq][Hq][D] with element strides, lse f32 [B][Hq][Sq] (may be NULL).  A workgroup owns PREFILL_QB query rows of one (b, query head)
// and walks the key tiles of PREFILL_KT keys up to its diagonal.  D in {64, 128}; one launch, no workspace, no atomics.
constexpr int PREFILL_QB = 256, PREFILL_KT = 32, PREFILL_MAX_SKV = 1 << 30;
inline int prefill_qblocks(int Sq) { return (int)(((long long)Sq + PREFILL_QB - 1) / PREFILL_QB); }
struct PrefillArgs {
  const void* q; long long q_sb, q_sh, q_ss;
  const void* k; long long k_sb, k_sh, k_ss;
  const void* v; long long v_sb, v_sh, v_ss;
  const unsigned char* mask; long long mask_sb;
  int B, Hq, G, Sq, Skv, q_offset;              // G = Hq / Hkv
  float scale;
  void* out; long long o_sb, o_ss, o_sh;
  float* lse;
};
int launch_prefill_attention(const PrefillArgs& a, int D, int op_dtype, hipStream_t stream);
// Its backward (prefill_attn_bwd.hip): out, dout [B][Sq][Hq][D], lse f32 [B][Hq][Sq] of the forward, dq as q, dk / dv as k / v, all with
// element strides; delta f32 [B][Hq][Sq] is the workspace.  Two launches: dQ (a workgroup owns PREFILL_BWD_QB query rows of one (b, query
// head), walks the key tiles up to its diagonal and writes delta), then dK / dV (a workgroup owns PREFILL_BWD_KB keys of one (b, K/V head)
// and walks the group's query heads in ascending order, each over the PREFILL_BWD_QT-row query tiles from its diagonal on).  No atomics.
constexpr int PREFILL_BWD_QB = 128, PREFILL_BWD_KB = 128, PREFILL_BWD_QT = 32;
struct PrefillBwdArgs {
  const void* q; long long q_sb, q_sh, q_ss;
  const void* k; long long k_sb, k_sh, k_ss;
  const void* v; long long v_sb, v_sh, v_ss;
  const unsigned char* mask; long long mask_sb;
  const void* out; long long o_sb, o_ss, o_sh;
  const void* dout; long long do_sb, do_ss, do_sh;
  const float* lse;
  int B, Hq, G, Sq, Skv, q_offset;              // G = Hq / Hkv
  float scale;
  void* dq; long long dq_sb, dq_sh, dq_ss;
  void* dk; long long dk_sb, dk_sh, dk_ss;
  void* dv; long long dv_sb, dv_sh, dv_ss;
  float* delta;
};
int launch_prefill_attention_backward(const PrefillBwdArgs& a, int D, int op_dtype, hipStream_t stream);
// The one-token step of the LM's decode (lm_step.hip): a skinny weight-streaming GEMM y [B][N] = x [B][K] W[N][K]^T for B <= LM_MAX_B rows
// with its prologue launch (RMSNorm to an fp32 copy, u = A x of up to three adapters), the embedding gather and the argmax with generate's
// greedy bookkeeping.  A workgroup owns LM_CB columns (rotary form: one head of D columns); W is read as stored and never copied.
constexpr int LM_MAX_B = 8, LM_MAX_R = 16, LM_MAX_EOS = 8, LM_CB = 16, LM_MAX_CB = 128;
enum LmEpi { LM_EPI_PLAIN = 0, LM_EPI_RES = 1, LM_EPI_SWIGLU = 2, LM_EPI_ROPE = 3 };
struct LmSeg {
  const void* W; long long ldw; int N;          // [N][K] operand dtype, pitch ldw
  int R; const float* Bw; const float* u; float scale;   // adapter: Bw [N][R], u [B][R] fp32 (R == 0: none)
  void* out; long long ldo;                     // [B][N]; SwiGLU writes segment 0's, the rotary form segment 0's (q) and the caches
};
struct LmSkinny {
  int B, K, nseg, epi, x_f32, out_f32;          // x_f32: x is the fp32 copy lm_prep left; out_f32: plain output in fp32
  const void* x; long long ldx;
  LmSeg seg[3];                                 // plain / residual: independent outputs; SwiGLU: gate, up; rotary: q, k, v
  const void* res; long long ldres;             // residual rows (may be the output)
  int Hq, Hkv, D, slot, pos_offset, rope_rows;  // rotary form: position[b] + pos_offset indexes cos / sin fp32 [rope_rows][rope_ld]
  const int* position; const float* cos; const float* sin; long long rope_ld;
  void* kc; void* vc; long long k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;   // caches [B][Hkv][Smax][D] with element strides; slot `slot` is written
  int cb, nblk[3];                              // set by the launch function
};
struct LmPrep {
  int B, K; const void* x; long long ldx;       // operand dtype rows
  const void* gain; float eps; float* xn;       // gain (operand dtype) NULL: no norm, u is taken from x itself; xn fp32 [B][K] dense
  const float* A[3]; int R[3]; float* u[3];     // A [R][K] fp32 -> u [B][R] fp32
};
struct LmGreedy {
  int* tokens_out; int* finished;               // [B] int32 each; finished NULL: plain argmax
  int pad, n_eos, eos[LM_MAX_EOS];
};
int launch_lm_embed(const int* tokens, const void* table, long long ld, int V, int B, int K, void* h, long long ldh, int op_dtype, hipStream_t stream);
int launch_lm_prep(const LmPrep& p, int op_dtype, hipStream_t stream);
int launch_lm_skinny(const LmSkinny& p, int op_dtype, hipStream_t stream);
int launch_lm_argmax(const float* logits, long long ld, int B, int V, const LmGreedy& g, hipStream_t stream);
// Row gather with a cast (prompt.hip): out [n_rows][width] (out_dtype 0 / 1 / 2 = f32 / f16 / bf16, pitch ldo) row i = source plan[i][0], row
// plan[i][1]; source -1 -> +0, any other entry out of range -> NaN, nothing read.  The per-source arguments are host arrays of n_src <=
// GATHER_MAX_SRC entries; plan int32 [n_rows][2] on the device.  width % 8 == 0, 16-byte aligned rows everywhere; a wave owns a row, no atomics.
constexpr int GATHER_MAX_SRC = 4;
int launch_gather_rows(void* out, long long ldo, int out_dtype, int n_rows, int width, const void* const* src_ptr, const long long* src_ld,
                       const int* src_rows, const int* src_dtype, int n_src, const int* plan, hipStream_t stream);
// Backward of launch_modality_ln without an item index (enc_grad.hip): x [items][tokens][E] (x_dtype 0 / 1 / 2 = f32 / f16 / bf16), d_out fp32;
// d_x (may be NULL, may be d_out) is written, d_gain / d_bias [E] (each may be NULL) are ADDED to.  E a multiple of 8, <= 4096.
int launch_modality_ln_bwd(const void* x, int x_dtype, int items, int tokens, int E, const float* gain, float eps, const float* d_out, float* d_x,
                           float* d_gain, float* d_bias, hipStream_t stream);
// db[n] (+)= sum_m dY[m][n]
int launch_colsum(const void* dY, long long block_stride, RowView yv, int M, int N, float* db, int accumulate, int op_dtype,
                  hipStream_t stream);

// ---- backward-pass row / elementwise / attention kernels (backward.hip) ----------------------------
struct LnBwdArgs {
  const float* dy; RowView dyv;   // upstream gradient of the LayerNorm output
  const float* x; RowView xv;     // saved pre-LN rows (statistics are recomputed)
  const float* gamma;
  float eps;
  int rows;
  float* dx; RowView dxv;         // gradient w.r.t. the pre-LN rows (+ `add` when given)
  const float* add; RowView addv; // optional second gradient stream added into dx (the residual branch)
  void* dx16; RowView dx16v;      // optional operand-dtype copy of dx
  float* dgamma; float* dbeta;    // optional, accumulated with float atomics
};
int launch_ln_bwd(const LnBwdArgs& a, int H, int op_dtype, hipStream_t stream);
// two independent LayerNorm backward jobs in one launch (b may be null or empty): the query-row and the text-row LayerNorm of a Q-Former layer
int launch_ln_bwd2(const LnBwdArgs& a, const LnBwdArgs* b, int H, int op_dtype, hipStream_t stream);
// out = gelu_erf(u) (backward = 0) or out = df * gelu'(u) (backward = 1); operand dtype, n % 8 == 0
int launch_gelu(const void* u, const void* df, void* out, long long n, int backward, int op_dtype, hipStream_t stream);
struct AttnBwdArgs {
  const void *Q, *K, *V, *O, *dO;   // operand dtype; O / dO share the [item][q row][head*64 + d] layout
  void *dQ, *dK, *dV;               // operand dtype; same layouts as Q / K / V (own strides)
  long long q_item_stride, o_item_stride, dq_item_stride;
  int q_ld, o_ld, dq_ld;
  long long k_item_stride, k_head_stride, v_item_stride, v_head_stride;
  int k_ld, v_ld;
  long long dk_item_stride, dk_head_stride, dv_item_stride, dv_head_stride;
  int dk_ld, dv_ld;
  const long long* mask; int mask_ld;
  const float* lse;                 // [item][head][q_rows] from the forward
  int items, heads, q_rows, kv_len;
  float scale;
  // several chain items behind one K/V item (mra_qformer_backward_multi): with kv_share = P > 1, `items` counts chain items (a multiple of P),
  // chain items n P .. n P + P - 1 read K / V item n and their dK / dV are summed into dK / dV item n; Q, O, dO, dQ, lse per chain item; no mask.
  // 0 or 1: every item its own K / V.
  int kv_share;
};
int launch_attn_bwd(const AttnBwdArgs& a, int op_dtype, hipStream_t stream);
// LDS of the backward core: the fp32 dQ / lse / delta areas grow with kv_share * ceil(q_rows / 32) query blocks; launch_attn_bwd refuses (-1) past the limit
constexpr size_t ATTN_BWD_LDS_LIMIT = 160 * 1024;
size_t attn_bwd_mfma_lds_bytes(int q_rows, int kv_share);
int attn_bwd_max_share(int q_rows);   // largest kv_share the LDS holds at q_rows (14 at q_rows <= 32); 0: q_rows itself is too long
#ifdef MRA_GEMM_EXPERIMENTS
void attn_bwd_force_valu(int on);   // A/B switch (experiment library only): the first (fp32 VALU) kernel instead of the MFMA one
#endif
int launch_embed_bwd(const float* demb, const long long* ids, int items, int L, int Q, int H, int vocab, float* dquery, float* dpos,
                     float* dword, hipStream_t stream);
int launch_transpose16(const void* src, void* dst, int R, int C, int op_dtype, hipStream_t stream);
// many transposes in one launch: job j owns the 32x32 tiles [tile_begin, next job's tile_begin) of its matrix
struct TrJob { const void* src; void* dst; int R, C, tile_begin, tiles_x; };
int launch_transpose16_batch(const TrJob* jobs_dev, int njobs, int total_tiles, int op_dtype, hipStream_t stream);
int launch_add_f32(const float* x, float* y, long long n, hipStream_t stream);  // y += x
struct FlatSeg;
// Fused optimizer pass of the training step (backward.hip): torch.optim.Adam's update on the flat fp32 master / gradient / moment buffers AND
// the refresh of the device weights it makes stale, in one read of each: per element  g += wd p;  m = b1 m + (1 - b1) g;
// v = b2 v + (1 - b2) g^2;  p -= step_size m / (sqrt(v) inv_sqrt_bc2 + eps);  then p goes out in the stored dtype (and, for the matrices
// with a transposed training copy, transposed as well through a 64 x 64 LDS tile); zero_grad clears g on the way.
struct AdamScalars { float beta1, beta2, eps, weight_decay, step_size, inv_sqrt_bc2; int zero_grad; };
struct AdamMatJob { unsigned long long off; void* dst; void* dstT; int R, C, ldT, tile_begin, tiles_x; };   // master offset (elements); dstT[c * ldT + r]
int launch_adam_mats(float* master, float* grad, float* m, float* v, const AdamMatJob* jobs_dev, int njobs, int total_tiles, AdamScalars sc, int op_dtype,
                     hipStream_t stream);
int launch_adam_flat(float* master, float* grad, float* m, float* v, const FlatSeg* segs, int nseg, AdamScalars sc, hipStream_t stream);

// ---- folded cross-attention helpers (fold.hip) ------------------------------------------------------
// P[row][0..kv) = softmax(scale * S[row][0..kv)) in the operand dtype, P[row][kv..kvp) = 0
int launch_softmax_rows(const float* S, long long ld_s, void* P, long long ld_p, int rows, int kv, int kvp, float scale, int op_dtype,
                        hipStream_t stream);
// second half of the split softmax (first half: EPI_SOFTPART of the scores GEMM): row statistics over the column tiles,
// then P[row][k] *= exp2(m_tile - m_row) / sum in place; columns [kv_cols, kvp) are zeroed.  tile_cols = columns per tile.
// split softmax, second half without a pass over P: factors[(row / R * ntiles + t) * 512 + row % R] = exp2(m_tile - m_row) / L_row from the
// tile statistics stat_*[row * ntiles + t] (rows = items * R, R <= 512); read by the P . enc GEMM through GemmProb::pscale.  Also zeroes
// the 16-bit P~ rows (row stride ld_p elements) from column ntiles * tile_cols to kvp, which the scores GEMM leaves unwritten.
// hist != nullptr: the probe variant, which also adds every row's softmax maximum 1 / L_row to the 256-bin histogram hist[256] of [0, 1]
// (automatic cross-attention precision); the factors and P~ are the same bits.
int launch_fold_rowfactor(const float* stat_m, const float* stat_l, float* factors, int rows, int R, int ntiles, void* P, long long ld_p, int tile_cols,
                          int kvp, hipStream_t stream, int* hist = nullptr);
// Steps 5 + 6a of a folded cross-attention layer in one launch (fold.hip: fold_query_kernel): Q_h = X W_cq,h^T + b_cq,h per head (X: M compact
// query rows behind the row view xv, K = H), rounded to the operand dtype, then Q'[item][head * Q + q][:] = Q_h W_k,h with Wk the per-head
// [E][64] blocks.  H and E multiples of 64, M a multiple of Q, head width 64; bit-identical to the two GEMM launches it replaces.
int launch_fold_query(const void* X, RowView xv, const void* Wq, const float* bq, const void* Wk, void* QP, int M, int H, int E, int Q, int heads,
                      int op_dtype, hipStream_t stream);
long long fold_rowfactor_launch_count();   // launch_fold_rowfactor launches (plain and probe) since the library was loaded
long long fold_query_launch_count();   // launches since the library was loaded (read-only diagnostics, as gemm_launch_count)
// hist != nullptr: the probe variant (as launch_fold_rowfactor's)
int launch_softmax_rescale(void* P, long long ld_p, const float* stat_m, const float* stat_l, int rows, int ntiles, int tile_cols, int kvp,
                           int op_dtype, hipStream_t stream, int* hist = nullptr);
// dst[b][c][r] = src[b][r][c] (r < R), 0 for R <= r < ld_d; src [batch][R][C], dst [batch][C][ld_d]
int launch_transpose_pad(const void* src, void* dst, int R, int C, int ld_d, long long src_bs, long long dst_bs, int batch, int op_dtype,
                         hipStream_t stream);

// The modality LayerNorm folded into a cross-attention weight (raw encoder features): row n of W [rows][E] (fp32 when w32, else the operand
// dtype) becomes w'_e = w_e g_e - mean_e(w g), computed in fp32 and rounded once -- W LN(x) = r (W' x) + W b with no mean term, because a
// centred row sums to zero.  key_layout: dst[(n / 64)][e][n % 64] (the per-head [heads][E][64] operand of the Q' GEMM), else dst[n][e].
// bias_out (may be null) [rows] = bias_in[n] + sum_e w_e b_e.
int launch_fold_ln_weight(const void* W, int w32, int rows, int E, const float* gain, const float* ln_bias, const float* bias_in, void* dst,
                          int key_layout, float* bias_out, int op_dtype, hipStream_t stream);

// ---- folded cross-attention, streaming form (fold_stream.hip) ---------------------------------------
// scores + split-softmax statistics + P . enc of one cross layer for `items` items of 384 (head, query) rows:
//   phase bit 0: P~ = exp2(alpha * Q' enc^T - ceil(tile max)) in f16 + per-(row, 176-column tile) statistics, then the row
//                statistics (tile factors 2^(m_tile - m_row) as f16, 1 / L);   phase bit 1: U = (1 / L) sum g P~ enc.
struct FoldStreamArgs {
  const void* qp;    // Q' [items][384][E] f16, row-major (the per-head Q' GEMM's output)
  void* qpb;         // workspace of the same size: Q' re-packed into the row operand's blocked layout
  const void* enc;   // encoder tokens [items][kv][E] f16
  void* p;           // P~ [items][384 x kvp] f16 (workspace; blocked layout [row / 16][k / 8][16][8])
  void* u;           // U  [items][384][E] f16
  float* stat_m;     // [items * 384][fold_stream_stat_ld(kvp)]
  float* stat_l;
  void* gexp;        // f16 [items * 384][stat_ld]
  float* ginv;       // [items * 384]
  int items, kv, kvp, E;
  float alpha;
  int phase;         // 3 = both
};
bool fold_stream_supported(int rows, int E, int kv, int kvp, int op_dtype);
int fold_stream_stat_ld(int kvp);
int launch_fold_stream(const FoldStreamArgs& a, hipStream_t stream);

// ---- attention ------------------------------------------------------------------------------
struct AttnArgs {
  const void* Q;  // [item][q row][head*64 + d], op dtype
  const void* K;  // token rows of 64 elements
  const void* V;
  void* O;        // [item][q row][head*64 + d], op dtype
  long long q_item_stride, o_item_stride;  // elements
  int q_ld, o_ld;
  long long k_item_stride, k_head_stride;  // elements; token row stride = k_ld
  long long v_item_stride, v_head_stride;
  int k_ld, v_ld;
  const long long* mask;  // [item][mask_ld] int64 (1 = attend) or nullptr; additive (1-m) * -10000
  int mask_ld;
  int items, heads, q_rows, kv_len;
  float scale;   // 1/sqrt(64)
  // grid-level KV split (cross attention with long KV): partials in `part`, combined by a 2nd kernel
  int nsplit;
  float* part;   // [items*heads*qblocks][nsplit][32*64 + 64] f32
  float* lse;    // optional [item][head][q_rows] f32: log2-sum-exp2 of the scaled, masked scores (for the backward)
  // several prompts over one K/V stream (mra_qformer_forward_multi): item n reads the K/V of item n / kv_share; Q, O, mask, partials
  // and lse stay per item
  int kv_share = 1;
};
size_t attn_partial_bytes(int items, int heads, int q_rows, int nsplit);
int attn_pick_split(int items, int heads, int q_rows, int kv_len);
int launch_attention(const AttnArgs& a, int op_dtype, hipStream_t stream);
// The shared-stream core: a workgroup is one (K/V item, head, group of up to 4 of its kv_share prompt slots); its 4 waves each own the 32
// queries of one slot and all read the K/V tiles from ONE workgroup-shared LDS ring, so the K/V bytes leave L2 / HBM once per 4 prompts.
// a.items = K/V items x a.kv_share, a.q_rows <= 32, no mask, no lse; a.nsplit from attn_shared_pick_split, partials as attn_partial_bytes
// (merged by the same combine kernel).
int attn_shared_pick_split(int kv_items, int kv_share, int heads, int kv_len);
int launch_attention_shared(const AttnArgs& a, int op_dtype, hipStream_t stream);
// Steps 1 + 2 of a layer in one launch (attention.hip: qkv_attn_kernel; mra_qformer_set_option "self_fuse"): the fused Q|K|V projection of the
// rows X [N * S][H] by wqkv [3H][H] (+ bqkv) and the masked self-attention core over them, one workgroup per (two consecutive items, head); Q, K
// and V pass through LDS and never reach HBM.  ctx [N * S][H] gets what launch_gemm on a ring tile + launch_attention give, bit for bit.
// S in 1 .. 64, H = heads * 64; -1 for any other shape (qkv_attn_supported).
bool qkv_attn_supported(int S, int H, int heads);
int launch_qkv_attention(const void* X, const void* wqkv, const float* bqkv, const long long* mask, void* ctx, int N, int S, int H, int heads,
                         int op_dtype, hipStream_t stream);
long long qkv_attn_launch_count();        // launches since the library was loaded (read-only diagnostics, as gemm_launch_count)
long long attn_launch_count(int masked);  // launch_attention launches of the one-wave-per-unit core: masked (self-attention) / not

// ---- normalisation / embeddings / conversions -----------------------------------------------
// y = LN(x) over H (multiple of 256, <= 1024) with gain/bias; writes f32 and/or op-dtype copies.
int launch_ln_rows(const float* x, RowView xv, int rows, int H, const float* gain, const float* bias, float eps,
                   float* y32, RowView y32v, void* y16, RowView y16v, int op_dtype, hipStream_t stream);
// as launch_ln_rows, but rows with (row % period) >= split use (gain2, bias2): the query and the text LayerNorm
// of a Q-Former layer in one launch over all rows of the [items, 32 + L, H] stream
int launch_ln_rows2(const float* x, RowView xv, int rows, int H, const float* gain, const float* bias, const float* gain2,
                    const float* bias2, int period, int split, float eps, float* y32, RowView y32v, void* y16, RowView y16v,
                    int op_dtype, hipStream_t stream);
// two Q-Formers in one launch (pair forward): rows [0, lane_rows) as launch_ln_rows2 with sets (1, 2), rows from lane_rows on with sets (3, 4)
// (gain4 == nullptr: set 3 for all of them)
int launch_ln_rows4(const float* x, RowView xv, int rows, int H, const float* gain, const float* bias, const float* gain2, const float* bias2,
                    int lane_rows, const float* gain3, const float* bias3, const float* gain4, const float* bias4, int period, int split,
                    float eps, float* y32, RowView y32v, void* y16, RowView y16v, int op_dtype, hipStream_t stream);
// Modality LayerNorm (A2) fused with the item gather (A3): out item i <- LN(in item index[i]).
// x dtype: 0 = f32, 1 = f16, 2 = bf16.
int launch_modality_ln(const void* x, int x_dtype, const long long* item_index, int items, int tokens, int E,
                       const float* gain, const float* bias, float eps, void* out, int op_dtype, hipStream_t stream);
// Embeddings (A4a): h[n, s] = LN(s < Q ? query[s] : word[ids[n, s-Q]] + pos[s-Q])
// query: [1 or items][Q][H]; query_item_stride = 0 broadcasts one set of query tokens to every item
int launch_embed_ln(const long long* ids, int items, int L, int Q, int H, int vocab, const float* query,
                    long long query_item_stride, const float* word,
                    const float* pos, const float* gain, const float* bias, float eps, float* h32, void* h16,
                    float* pre32 /* optional: rows before the LayerNorm (training) */, int op_dtype, hipStream_t stream);
// dst(op dtype)[rows][cols] at row offset <- src (0 = f32, 1 = f16, 2 = bf16)
// One launch that refreshes many parameters from a flat f32 master buffer: segment s copies / converts
// n (<= FLAT_SEG) elements from master + src_off to dst in the stored dtype (0 f32, 1 f16, 2 bf16).
struct FlatSeg { unsigned long long src_off; void* dst; int n; int dtype; };
constexpr int FLAT_SEG = 16384;
int launch_convert_flat(const float* master, const FlatSeg* segs, int nseg, hipStream_t stream);
int launch_convert(const void* src, int src_dtype, void* dst, int dst_dtype /*0 f32,1 f16,2 bf16*/, long long n,
                   hipStream_t stream);
int launch_copy_rows_f32(const float* src, RowView sv, float* dst, RowView dv, int rows, int H, hipStream_t stream);
// split-precision cross-attention: fp32 -> operand-dtype (hi, lo) pairs laid out for K-concatenated GEMMs (norm_embed.hip)
//   rows:   dst[row][c / chunk][part][c % chunk], parts = 3: (hi, lo, hi), 2: (hi, lo); dense dst rows of C * parts elements
//   weight: [rows][C] -> [rows][3 C] = (hi | hi | lo);  key weight: [heads * 64][E] -> [heads][E][192] = (hi | hi | lo) over the head dims
int launch_split_rows(const float* src, RowView sv, int rows, int C, int chunk, int parts, void* dst, int op_dtype, hipStream_t stream);
int launch_split_weight(const float* W, int rows, int C, void* dst, int op_dtype, hipStream_t stream);
int launch_split_key_weight(const float* W, int heads, int E, void* dst, int op_dtype, hipStream_t stream);

// Allows kernel `fn` `lds` bytes of dynamic LDS on the current device: hipFuncSetAttribute once per (kernel, device), under a mutex (gemm.hip).
// Not a stream operation: call it before the launch, outside any stream capture.  false: the runtime refused.
bool ensure_lds(const void* fn, size_t lds);

// ---- scorer -------------------------------------------------------------------------------------
int launch_cosine_score(const float* z, const float* t, int t_rows, int items, int Q, int H, float eps, float* sim,
                        float* logit, hipStream_t stream);
int launch_fuse_logits(const float* const* logits, const float* weights, int nmod, int n, float* out,
                       hipStream_t stream);
int launch_span(const float* logits, int videos, int clips, float alpha, int* spans, hipStream_t stream);
// windows.hip: ranked top-k windows under temporal NMS (include/mra.h: mra_windows_from_logits); clips 1..4096, top_k 1..64
int launch_windows(const float* logits, int videos, int clips, float alpha, int top_k, float nms_thd, int max_len, int* windows,
                   float* scores, int* counts, hipStream_t stream);

}  // namespace mra
