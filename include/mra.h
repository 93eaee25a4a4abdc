/* mra.h -- C ABI of the MI355X (gfx950) cross-modal encode/fuse/score hot path of mrAudio.
 *
 * The reference (globc/mrAudio) is pure Python and has no FFI; the boundary this library stands
 * behind is the duck-typed seam inside XInstructBLIP.generate()/forward():
 *     ln(encoder(frame))                                   models/xinstructblip.py:265,274,822-828
 *     cat(embeds)[indices]                                 models/xinstructblip.py:281-285
 *     {modality}_Qformer.bert(input_ids, attention_mask=, query_embeds=,
 *                             encoder_hidden_states=, encoder_attention_mask=)   :286-293
 *     {modality}_llm_proj(last_hidden_state[:, :32, :])    models/xinstructblip.py:303
 * plus the similarity scorer the north star adds in place of the LLM decode (no reference site).
 * Each entry point below names the reference call it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every data pointer is a DEVICE pointer on the handle's GPU;
 *   - the caller (PyTorch) owns every buffer, including the workspace; after create/load the
 *     library never allocates device memory and never synchronises the stream;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*, NULL = default stream);
 *   - return 0 on success, a negative MRA_E* code otherwise; mra_last_error() gives the text;
 *   - a handle is bound to the device that was current at create; calls on one handle are not
 *     re-entrant, distinct handles are independent (one per rank / modality).  One exception: after
 *     mra_qformer_prepare, several mra_qformer_forward calls of one handle may be in flight on different
 *     streams (they only read the handle; each needs its own workspace and outputs);
 *   - tensors are dense row-major; matrices of nn.Linear are [out, in] as PyTorch stores them.
 */
#ifndef MRA_H_
#define MRA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRA_OK 0
#define MRA_EINVAL (-1)    /* bad argument / unsupported shape */
#define MRA_ESTATE (-2)    /* weights missing, handle not finalised ... */
#define MRA_EHIP (-3)      /* a HIP call failed */
#define MRA_ENOMEM (-4)    /* workspace too small / allocation failed */
#define MRA_ENAME (-5)     /* unknown weight name */

/* element types */
#define MRA_F32 0
#define MRA_F16 1
#define MRA_BF16 2

typedef struct mra_qformer mra_qformer;

/* Shape of one modality Q-Former; defaults = reference models/xinstructblip.py:614-627
 * (bert-base-uncased + cross-attention every 2nd layer, 32 queries, vocab 30522 + [DEC]). */
typedef struct mra_cfg {
  int32_t hidden;      /* 768; multiple of 256, <= 1024 */
  int32_t heads;       /* 12; hidden / heads must be 64 */
  int32_t inter;       /* 3072 */
  int32_t layers;      /* 12 */
  int32_t cross_freq;  /* 2: layers i % cross_freq == 0 carry cross-attention */
  int32_t enc_width;   /* 1408 (EVA ViT-g) / 768 (BEATs); multiple of 64 */
  int32_t n_query;     /* 32 (fixed by the kernels) */
  int32_t vocab;       /* 30523 */
  int32_t max_pos;     /* 512 */
  float ln_eps;        /* 1e-12 (BERT LayerNorm) */
  float enc_ln_eps;    /* 1e-5  (modality LayerNorm, torch default) */
  int32_t llm_hidden;  /* 4096 (a multiple of 64), or 0 when no llm_proj is loaded */
  int32_t op_dtype;    /* MRA_F16 (default, the reference's autocast dtype) or MRA_BF16: MFMA operand type */
} mra_cfg;

/* Fills *cfg with the reference defaults for the given encoder width. */
void mra_cfg_default(mra_cfg* cfg, int32_t enc_width);

const char* mra_last_error(void);
const char* mra_version(void);

/* ---- lifetime -------------------------------------------------------------------------------
 * replaces: XInstructBLIP.init_Qformer / init_ln / init_vicuna_projection
 * (models/xinstructblip.py:614-655,678-735): construction + weight loading. */
int mra_qformer_create(const mra_cfg* cfg, mra_qformer** out);
void mra_qformer_destroy(mra_qformer* h);

/* Copies (and converts to the operand dtype) one parameter.  `name` uses the LAVIS checkpoint keys
 * with the leading "{modality}_Qformer." stripped, as the reference's loader does
 * (models/xinstructblip.py:647-652): "bert.embeddings.word_embeddings.weight",
 * "bert.encoder.layer.3.attention.self.query.weight", "...crossattention.output.LayerNorm.bias",
 * "...intermediate_query.dense.weight" ... plus "query_tokens" ({m}_query_tokens),
 * "ln.weight"/"ln.bias" ({m}_ln.*), "llm_proj.weight"/"llm_proj.bias" ({m}_llm_proj.*).
 * src is a device pointer of `dtype` with `ndim` dims `shape`.  Unknown name -> MRA_ENAME. */
int mra_qformer_load(mra_qformer* h, const char* name, const void* src, int32_t dtype, const int64_t* shape,
                     int32_t ndim, void* stream);
/* Number of parameters still missing (0 = ready); names are written comma separated into buf. */
int mra_qformer_missing(mra_qformer* h, char* buf, size_t buflen);

/* ---- A2 + A3: modality LayerNorm fused with the sample-major reorder ---------------------------
 * replaces: ln(encoder(frame)) and torch.cat(embeds)[indices]
 * (models/xinstructblip.py:265,274,281-285,822-828).
 * x [n_src_items, tokens, enc_width] of x_dtype; item_index [items] int64 (NULL = identity) gives,
 * for every output item, the source item; out [items, tokens, enc_width] in the operand dtype. */
int mra_modality_ln(mra_qformer* h, const void* x, int32_t x_dtype, const int64_t* item_index, int32_t items,
                    int32_t tokens, void* out, void* stream);

/* ---- A4: Q-Former forward -----------------------------------------------------------------------
 * replaces: {modality}_Qformer.bert(input_ids.repeat(T,1), attention_mask=..., query_embeds=
 * query_tokens.repeat(T,1,1), encoder_hidden_states=..., encoder_attention_mask=ones)
 * (models/xinstructblip.py:286-293).  The learned query tokens are the loaded "query_tokens"
 * (the reference tiles the same [1,32,H] parameter for every item); encoder_attention_mask is
 * all ones in the reference and is not an input here.
 *   input_ids      [items, L] int64
 *   attention_mask [items, n_query + L] int64 (1 = attend) or NULL = all ones
 *   query_embeds   [query_items, n_query, hidden] f32 with query_items == 1 (broadcast) or == items,
 *                  or NULL = the loaded "query_tokens" parameter
 *   enc            [items, kv, enc_width] operand dtype (output of mra_modality_ln)
 *   out_query      [items, n_query, hidden] f32 = last_hidden_state[:, :32, :]        (required)
 *   out_full       [items, n_query + L, hidden] f32 = last_hidden_state, or NULL
 *   out_cls        [items, hidden] f32 = last_hidden_state[:, 32, :], or NULL (needs L >= 1)
 * When neither out_full nor out_cls is given the last layer's text feed-forward is skipped
 * (its result is never read by the reference either: only [:, :32] is sliced, :303). */
size_t mra_qformer_workspace_bytes(mra_qformer* h, int32_t items, int32_t L, int32_t kv);
int mra_qformer_forward(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask,
                        const float* query_embeds, int32_t query_items, const void* enc, int32_t items, int32_t L,
                        int32_t kv, float* out_query, float* out_full, float* out_cls, void* workspace,
                        size_t workspace_bytes, void* stream);

/* The same forward over RAW encoder features: `enc` [items, kv, enc_width] is what mra_modality_ln would READ (operand dtype, contiguous,
 * no item gather), and no normalised copy is made.  The modality LayerNorm lives in the folded cross-attention instead: its gain and the
 * centring inside the key / value weights (W' = W diag(g) with every row centred over enc_width, so W LN(x) = r (W' x) + W b and the token
 * mean never appears), its bias inside the value bias, and the token factors r = 1 / sqrt(var + enc_ln_eps) are computed by cross layer 0's
 * scores launch from the token rows as they stream through its LDS, applied to the score columns, and kept in the workspace for the
 * later cross layers.  Only the folded form on the 176 x 384 tiles with in-register row factors, in operand precision:
 *   mra_qformer_raw_features_ok(h, kv, x_dtype)   1 when a forward of h over kv tokens per item of dtype x_dtype can take raw features --
 *       folded form (cross mode 2, or 0 with kv >= 2048; not the streaming kernels, not the separate rescale pass), heads * n_query == 384,
 *       enc_width a multiple of 176, x_dtype the operand dtype, ln.weight and ln.bias loaded, no split precision and no pending or
 *       split-resolved automatic precision, and mra_qformer_set_option "raw_features" not 0.  Otherwise 0: run mra_modality_ln and
 *       mra_qformer_forward, whose results do not change.
 *   mra_qformer_forward_raw   arguments, checks and workspace as mra_qformer_forward; MRA_ESTATE where mra_qformer_raw_features_ok says 0.
 * The folded weights are rounded to the operand dtype AFTER centring, so a token's mean mu meets their rounding error uncancelled: against
 * the normalised-copy path the scores err by about 2^-11 |mu| / sigma relative (f16) on top of the operand rounding both paths share.
 * Features whose mean over enc_width is many standard deviations from zero are better served by mra_modality_ln. */
int mra_qformer_raw_features_ok(mra_qformer* h, int32_t kv, int32_t x_dtype);
int mra_qformer_forward_raw(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask,
                            const float* query_embeds, int32_t query_items, const void* enc, int32_t items, int32_t L,
                            int32_t kv, float* out_query, float* out_full, float* out_cls, void* workspace,
                            size_t workspace_bytes, void* stream);

/* The dominant launch of the forward on its own (what bench.py prices against the MFMA roofline):
 * K and V of every cross-attention layer, enc [items*kv, enc_width] x Wkv[n_cross*2*hidden, enc_width]^T
 * + bias, written head-major into kv_cache [n_cross][2][items][heads][kv][64] (operand dtype,
 * mra_kv_cache_bytes).  mra_qformer_forward performs exactly this launch as its second step. */
size_t mra_kv_cache_bytes(mra_qformer* h, int32_t items, int32_t kv);
int mra_kv_project(mra_qformer* h, const void* enc, int32_t items, int32_t kv, void* kv_cache, void* stream);

/* Two Q-Formers of equal shape (hidden / heads / inter / layers / cross_freq / n_query / operand dtype) over the SAME prompt in one launch
 * sequence: replaces the two `{m}_Qformer.bert(...)` calls of one step (models/xinstructblip.py:286-293, once per modality).  The layer
 * chains -- identical in shape for every modality -- run as grouped launches (each chain GEMM takes both lanes' problems, the self-attention
 * cores and LayerNorms take the 2 x items rows as one launch); each lane keeps its own cross-attention (encoder width, Kv and formulation may
 * differ).  A chain launch at ~2 k rows is half fixed cost: the grouped sequence spends 0.7 ms less kernel time per
 * headline step and its folded blocks run undisturbed (0.65 instead of 0.79 ms) -- but two forwards on two streams hide ~0.65 ms of the light
 * modality behind the heavy one's latency-bound phases, which one sequence cannot: measured 6.72-6.87 vs 6.57 ms per step.  Kept as a
 * tested alternative (Python: model.pair_forward = True).  Same arithmetic per lane as mra_qformer_forward
 * (learned query tokens, operand-dtype score chain); outputs: out_query [items, 32, H] and / or out_cls [items, H] per lane (fp32).
 * Workspace: mra_qformer_pair_workspace_bytes. */
size_t mra_qformer_pair_workspace_bytes(mra_qformer* h0, mra_qformer* h1, int32_t items, int32_t L, int32_t kv0, int32_t kv1);
int mra_qformer_forward_pair(mra_qformer* h0, mra_qformer* h1, const int64_t* input_ids, const int64_t* attention_mask, const void* enc0,
                             const void* enc1, int32_t items, int32_t L, int32_t kv0, int32_t kv1, float* out_query0, float* out_cls0,
                             float* out_query1, float* out_cls1, void* workspace, size_t workspace_bytes, void* stream);
/* The same with RAW encoder features for the lanes whose bit is set in raw_mask (bit 0: enc0, bit 1: enc1), each as mra_qformer_forward_raw
 * takes them (MRA_ESTATE where mra_qformer_raw_features_ok says 0 for that lane); raw_mask 0 is mra_qformer_forward_pair.  Per lane the
 * launches and the results are those of the lane's own mra_qformer_forward / mra_qformer_forward_raw call. */
int mra_qformer_forward_pair_raw(mra_qformer* h0, mra_qformer* h1, const int64_t* input_ids, const int64_t* attention_mask, const void* enc0,
                                 const void* enc1, int32_t raw_mask, int32_t items, int32_t L, int32_t kv0, int32_t kv1, float* out_query0,
                                 float* out_cls0, float* out_query1, float* out_cls1, void* workspace, size_t workspace_bytes, void* stream);

/* Multi-prompt forward: `prompts` prompts per encoder item over ONE shared K/V cache.
 * replaces: model.{modality}_Qformer.bert(...) (models/xinstructblip.py:286-293) as evaluate.py:42-44 calls it once per (vid, query)
 * annotation line -- P lines of one video become one call with prompts = P, and the encoder rows of the video are given once.
 *   input_ids      [enc_items * prompts, L]       int64   row i * prompts + p: encoder item i, prompt slot p; prompts differ freely per row
 *   attention_mask [enc_items * prompts, 32 + L]  int64   same row order, or NULL (all ones)
 *   enc            [enc_items, kv, E]             operand dtype, as mra_modality_ln writes it; the learned query tokens are the loaded parameter
 *   out_query      [enc_items * prompts, 32, H]   fp32 (may be NULL)
 *   out_cls        [enc_items * prompts, H]       fp32 (may be NULL; needs L >= 1)
 * The layer chain runs on enc_items * prompts items; the K/V projection runs once on enc_items items and the cross core of chain item n
 * reads the K/V of item n / prompts.  Always the K/V-cache form in operand precision, whatever mra_qformer_set_cross_mode says: per cross
 * layer and encoder item the projection costs 4 Kv E 768 flops (call it 1), the folded form 0.5 per prompt, the flash core over a cache
 * 4 384 Kv 64 = 0.023 per prompt at E = 1408 -- so P prompts cost 0.5 P folded, 1.023 P with a cache re-projected per replica and
 * 1 + 0.023 P here (fewer flops from P = 3; arithmetic, not a measurement).  The cross core follows mra_qformer_set_option "multi_core".
 * Precision as mra_qformer_forward_pair: MRA_ESTATE while split precision is in force or automatic precision is unresolved or resolved to
 * split.  Argument checks as mra_qformer_forward, plus prompts >= 1; enc_items == 0 is a no-op; no allocation, no synchronisation;
 * prompts == 1 is the K/V-cache mra_qformer_forward launch for launch.  Workspace: mra_qformer_multi_workspace_bytes (0 for a NULL
 * handle or a non-positive size), 256-byte aligned. */
size_t mra_qformer_multi_workspace_bytes(mra_qformer* h, int32_t enc_items, int32_t prompts, int32_t L, int32_t kv);
int mra_qformer_forward_multi(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask, const void* enc,
                              int32_t enc_items, int32_t prompts, int32_t L, int32_t kv,
                              float* out_query, float* out_cls, void* workspace, size_t workspace_bytes, void* stream);

/* Optional instrumentation for bench.py: when both events (hipEvent_t passed as void*) are non-NULL,
 * every following mra_qformer_forward records ev_start right before and ev_stop right after its
 * K/V-projection launch, on the launch stream.  (NULL, NULL) switches it off. */
int mra_qformer_set_kv_events(mra_qformer* h, void* ev_start, void* ev_stop);

/* How the six cross-attention layers are computed (HF modeling_instructblip.py:464-515 arithmetic either way):
 *   1  K/V cache: K and V of every cross layer projected up front by one GEMM, then a flash-style core per layer;
 *   2  folded:    per layer S = (Q W_k) enc^T, P = softmax(S / 8), context = (P enc) W_v^T + b_v -- half the flops
 *                 at any Kv (the 32 queries are fewer than the 64 head dimensions).  With 12 heads and enc_width % 176 == 0
 *                 the two big products run on the 176 x 384 loader-wave GEMM tile with the softmax split over the
 *                 176-column tiles: tile statistics in the scores epilogue, row factors exp2(m_tile - m_row) / L from a
 *                 small kernel, applied by the P . enc GEMM to its P~ fragments on their way into the MFMA (P is written
 *                 once and read once); otherwise on 128 x 128 tiles with fp32 score rows;
 *   0  automatic (default): folded from Kv >= 2048;
 *   3  as 2 on the 128 x 384 loader-wave tile (A/B runs: no faster);
 *   4  as 2 on the streaming kernels of fold_stream.hip (f16 only: row operands straight to registers two K steps
 *      ahead, slab ring of four LDS slots, power-of-two tile factors applied in registers, no rescale pass).  Measured
 *      13 % SLOWER than mode 2 -- both forms sit on the per-CU load path, DESIGN.md section 8 -- kept, tested, opt-in.
 *   5  as 2 with the row factors applied by a separate rescale pass over P (the round-1 form; same results bit for bit, one more
 *      read and write of P per layer: kept as the measured alternative).
 * mra_qformer_workspace_bytes follows the mode in force; the training entry points always use the K/V cache. */
int mra_qformer_set_cross_mode(mra_qformer* h, int32_t mode);
/* Precision of the cross-attention SCORE chain (no reference counterpart: the reference runs it in fp16 under autocast,
 * models/xinstructblip.py:58-66; its CPU path in fp32):
 *   0  (default) MFMA operands in the operand dtype: the hidden state, W_cq, Q, W_k and Q' = Q W_k are each rounded to 11 bits.
 *      A peaked softmax amplifies that rounding (dp = p (1 - p) ds, |s| up to ~100 for trained, sharply attending Q-Formers);
 *   1  split: every operand of the chain hidden -> Q -> Q' -> scores is carried as an operand-dtype hi + lo pair (~22 bits with
 *      f16): x.w = [xh | xl | xh].[wh | wh | wl]^T on the ordinary GEMM kernels (K tripled on the two small projections), and the
 *      scores product reads Q' as (hi | lo) rows against the SAME encoder slab twice inside one K loop (K doubled, slab bytes
 *      unchanged).  Forces the folded form at any Kv; needs heads * n_query == 384.  The f32 copies of W_cq / W_k live in the parameter
 *      arena (kept current by mra_qformer_load / _load_flat); the first call with mode 1 allocates the prepared-weight arena
 *      (ncross x (3 H H + 3 H E) operand elements) -- the one allocation after create.  Cost and accuracy: DESIGN.md section 8.
 *   2  auto: 0 or 1, chosen on the GPU from how peaked the attention is.  Same preconditions as 1; allocates the
 *      split weight arena (and 2 x ncross x 1 KB of histograms, device and pinned host) up front and marks the probe stale, as do every
 *      mra_qformer_load / _load_flat / _adam_step and every further call with mode 2.  The first mra_qformer_forward with a stale probe runs
 *      the mode-0 folded chain (at any Kv and cross mode; never the streaming kernels, nor the rescale pass where enc_width % 176 == 0
 *      gives the in-register row factors) with the probe variant of the row-factor (or rescale) kernel, which bins every row's softmax maximum p_max = 1 / L into a 256-bin histogram per cross layer; it copies the
 *      histograms to the host and synchronises `stream` once (the only host sync, on this call only; it returns MRA_ESTATE "auto precision
 *      unresolved: run one forward outside capture" while the stream is capturing) and resolves to 1 iff the largest per-layer median p_max is
 *      >= tau, otherwise to 0.  Resolved to 1 -- or to 0 where mode 0 runs another form (the K/V cache, the streaming kernels) -- the same
 *      call re-runs the forward in the resolved precision: the outputs returned are always those of the precision in force from then on.  Later forwards run the resolved mode with no probe and no sync (resolved to 0: the kernels of
 *      mode 0 exactly).  tau = 0.5 by default (mra_qformer_set_option "auto_split_pmax_milli"): the mode-0 chain is measured inside the
 *      1e-3 similarity-logit bar at a median p_max of 0.6 (7.3e-4, worst formulation) and outside it at 0.8, so 0.5 keeps a margin and sends
 *      those 0.6 cases to split (peaked fixtures only -- no trained checkpoint was measured).  mra_qformer_forward_pair
 *      accepts the handle only once it resolved to 0 (MRA_ESTATE otherwise).  Governs inference forwards only: the training entry points
 *      run the mode-0 chain whatever the precision.
 * mra_qformer_workspace_bytes follows the precision in force; under 2 it returns the largest of the mode-0 form in force, the mode-0 folded
 * form of the probe and mode 1, so neither the probe nor its resolution needs a larger workspace. */
int mra_qformer_set_cross_precision(mra_qformer* h, int32_t mode);
/* State of the cross-attention precision (no reference counterpart: the reference has one fixed precision, fp16 under autocast,
 * models/xinstructblip.py:58-66).  resolved: 0 op / 1 split in force, -1 while an automatic-precision probe is pending; probes: probes run
 * since create (a steady state adds none); median_pmax (may be NULL, else n_layers >= the number of cross layers): per cross layer the
 * median softmax row maximum the last probe measured, at the centre of its 1/256 bin (-1 before any probe).  Any pointer may be NULL. */
int mra_qformer_cross_precision_report(mra_qformer* h, int32_t* resolved, int32_t* probes, float* median_pmax, int32_t n_layers);
/* Per-handle tuning options (no reference counterpart; results are the same to fp32 summation order).
 *   "chain_ring"  mask: which GEMMs of the 12-layer chain run on the ring kernel's exact-fit tiles when the launch has ~1 k rows or more:
 *                 bit 0 QKV (144 x 128), bit 1 FFN-up (192 x 128), bit 2 the residual projections (96 x 64), bit 3 (with bit 2) their LayerNorm inside the same
 *                 launch (the last-arriving column tile of a 64-row block normalises it).  DESIGN.md section 8.
 *   "train_ring"  the same mask (bits 0 and 2) for the GEMMs of mra_qformer_forward_train / mra_qformer_backward; default 4.
 *   "auto_split_pmax_milli"  tau of the automatic cross-attention precision in thousandths, 0..1000 (default 500); applies from the next probe.
 *   "raw_features"  1 (default): mra_qformer_raw_features_ok may answer yes; 0: it answers no (A/B against the normalised-copy path).
 *   "multi_core"  the cross core of mra_qformer_forward_multi with prompts > 1: 0 the core of mra_qformer_forward, each chain item taking the
 *                 K/V of its encoder item; 1 the shared-stream core (one workgroup per encoder item, head and 4 prompt slots, the K/V tiles
 *                 staged once into a workgroup-shared LDS ring).  Default 1 (faster at P >= 4 on both shapes of tools/bench_multi_query.py, by 0.2 - 2.3 %;
 *                 0 is 6 % ahead at P = 2, Kv 8224).  mra_qformer_multi_workspace_bytes follows it.
 *   "cross_fuse"  mask over the launches around the two big GEMMs of the folded cross-attention; only the default folded plan follows it (the
 *                 176 x 384 tiles with in-register row factors, operand precision, no probe; raw features or the normalised copy), every
 *                 other form keeps its launches.  1: cross query projection and per-head Q' in ONE launch (mra_debug_fold_query), Q is not
 *                 written; 4: the per-head context GEMM on the 64 x 64 tile with 128-deep K steps (enc_width % 128 == 0, >= 512 query
 *                 rows); 2: the row factors of the split softmax computed inside the P . enc launch from the scores launch's tile
 *                 statistics (no fold_rowfactor launch).  All bit-identical to mask 0, which issues the launches as before.  Default 1: the
 *                 only bit that measured a gain in the step.  Bit 4 measured no difference and bit 2 measured a loss (+0.30 ms per
 *                 step: the P . enc launch grows by more than the launch it absorbs); both stay as tested opt-ins.
 *   "self_fuse"   1: the Q|K|V projection and the masked self-attention core of every layer run as ONE launch (mra_debug_qkv_attention): Q, K
 *                 and V pass through LDS, the QKV array is neither written nor read.  Taken by single-lane forwards (mra_qformer_forward,
 *                 _forward_multi) with 32 + L <= 64 rows per item, 64-wide heads and a QKV GEMM on its ring tile ("chain_ring" bit 0, at
 *                 least 1024 rows in all): there it is bit-identical to the two launches.  The pair forward, longer prompts, smaller
 *                 forwards, forwards that return the full sequence (out_full) and the training forward keep the two launches.  0: the two launches everywhere.  Default 1: -0.08 to -0.11 ms per headline step, -0.16 ms at the reference item shape. */
int mra_qformer_set_option(mra_qformer* h, const char* name, int32_t value);
/* Derives what the folded path needs from the loaded weights (W_k of every cross layer regrouped per head) on
 * `stream`, if a load made it stale.  mra_qformer_forward does this itself; a caller that runs SEVERAL forwards of one
 * handle concurrently on different streams calls it once before forking. */
int mra_qformer_prepare(mra_qformer* h, void* stream);

/* Scheduling hook: when `ev` (hipEvent_t as void*) is non-NULL every following mra_qformer_forward records it
 * right after its K/V-projection launch, on the launch stream.  The host side makes the light modality's
 * stream wait for the heavy modality's event, so the chip-filling GEMM runs alone and the two latency-bound
 * layer chains overlap each other instead (mraudio_amd/models/xinstructblip.py: fuse_score).  NULL = off. */
int mra_qformer_set_kv_done_event(mra_qformer* h, void* ev);

/* ---- A5: LLM projection ---------------------------------------------------------------------------
 * replaces: {modality}_llm_proj(last_hidden_state[:, :32, :]) (models/xinstructblip.py:303).
 * z [rows, hidden] f32 -> out [rows, llm_hidden] of out_dtype (MRA_F32 or the operand dtype).
 * workspace: rows * hidden operand elements. */
int mra_llm_proj(mra_qformer* h, const float* z, int32_t rows, void* out, int32_t out_dtype, void* workspace,
                 size_t workspace_bytes, void* stream);
/* Backward of mra_llm_proj: the link that lets the language model's loss on the answer tokens reach the Q-Former.  Beyond the reference on
 * this path ({modality}_llm_proj at models/xinstructblip.py:303 is trained there only by torch autograd).  With y = op(z) W^T + b, op the
 * rounding to the operand dtype and dY = op(d_out):
 *   d_z [rows, hidden] f32       = dY W            WRITTEN.  One MFMA launch that reads W [llm_hidden, hidden] as stored through the LDS
 *                                                  transpose read (the kernel of mra_qformer_backward_enc on a row-major dY): no transposed
 *                                                  copy of the weight exists, so none can go stale; no atomics.
 *   d_weight [llm_hidden, hidden] f32 += dY^T op(z),   d_bias [llm_hidden] f32 += colsum(dY)     ADDED to, one launch for both (float atomics
 *                                                  where the contraction over rows is split: the order over rows is then not fixed).
 * z [rows, hidden] f32 is what the forward was given; d_out [rows, llm_hidden] is MRA_F32 (rounded to the operand dtype into the workspace
 * first; the rounding of z and d_out is passed straight through) or the handle's operand dtype (16-byte aligned).  Each of d_z, d_weight,
 * d_bias may be NULL and skips its work.  Nothing is written into the flat gradient buffer of mra_qformer_backward: its llm_proj.* slots stay
 * zero.  Checks, all before any launch: NULL handle, negative rows (rows == 0 is a no-op), llm_proj.* not loaded (MRA_ESTATE), llm_hidden not
 * a multiple of 64 or hidden not a multiple of 128, d_out_dtype, NULL z / d_out, rows * llm_hidden above int32 (MRA_EINVAL), workspace below
 * mra_llm_proj_backward_workspace_bytes (MRA_ENOMEM, naming the need; 0 for a NULL handle or non-positive rows, 256-byte aligned).
 * No allocation, no synchronisation. */
size_t mra_llm_proj_backward_workspace_bytes(mra_qformer* h, int32_t rows, int32_t d_out_dtype);
int mra_llm_proj_backward(mra_qformer* h, const float* z, int32_t rows, const void* d_out, int32_t d_out_dtype, float* d_z, float* d_weight,
                          float* d_bias, void* workspace, size_t workspace_bytes, void* stream);

/* ---- LoRA: the low-rank branch of one adapted linear of the attached LM ---------------------------------------
 * replaces: the peft LoraLayer branch the reference configures in models/model_utils.py:4-14 (r = 8, lora_alpha = 8, lora_dropout = 0.05,
 * bias "none") and applies at models/xinstructblip.py:163 -- restated from the published algorithm, unpinned to peft.  Stateless like
 * mra_cosine_score: caller-owned buffers, a stream, no allocation, no synchronisation.  With x [rows][K], y [rows][N] in `dtype` (MRA_F16 /
 * MRA_BF16; op = rounding to it), fp32 adapters A [R][K], B [N][R], s = alpha / R, q = 1 - p:
 *   forward   u = mra_lora_down(x, A as RN, scale 1/q, p, seed);   mra_lora_up_add(y = x W^T, u, B as NR, scale s, p 0)
 *   backward  du = mra_lora_down(dY, B as NR, scale s, p 0);        mra_lora_wgrad(dY, u -> dB as NR, scale s, p 0);
 *             mra_lora_wgrad(x, du -> dA as RN, scale 1/q, p, seed);   mra_lora_up_add(dx = dY W, du, A as RN, scale 1/q, p, seed)
 * A small fp32 matrix over (width index n, rank index j) is MRA_LORA_NR = [width][R] or MRA_LORA_RN = [R][width].  Dropout is counter based
 * and never stored: element (m, n) of a [rows][width] tensor is kept when lowbias32(lo32(i) ^ lo32(seed) ^ hi32(i) * 0x9E3779B9 ^ hi32(seed))
 * >= floor(p 2^32 + 0.5), i = m * width + n (the width, not the pitch); p == 0 hashes nothing.  The scale is applied as given (the caller
 * passes 1/q).  Checked before any launch (MRA_EINVAL): NULL pointers, R outside 1..16, a width that is not a positive multiple of 8, pointers or
 * pitches that are not 16-byte aligned, ld < width, p outside [0, 1), unknown dtype or layout, negative rows; rows == 0 is a no-op.
 *
 * out [rows][R] f32 (dense) = scale * drop(x)[rows][K] op(w)^T: matrix cores, fp32 accumulation, w rounded to `dtype` on its way in. */
#define MRA_LORA_NR 0
#define MRA_LORA_RN 1
int mra_lora_down(const void* x, int64_t ldx, int32_t rows, int32_t K, int32_t dtype, const float* w, int32_t R, int32_t w_layout, float scale,
                  double p, uint64_t seed, float* out, void* stream);
/* y [rows][N] (`dtype`, pitch ldy) = op(float(y) + scale * keep * sum_j u[m][j] w(n, j)) IN PLACE: an fp32 fma chain from 0 with j ascending, then
 * one fma onto float(y); a dropped element keeps its bits. */
int mra_lora_up_add(void* y, int64_t ldy, int32_t rows, int32_t N, int32_t dtype, const float* u, int32_t R, const float* w, int32_t w_layout,
                    float scale, double p, uint64_t seed, void* stream);
/* dw (f32, dw_layout) += scale * drop(x)[rows][N]^T op(u)[rows][R]: the contraction over rows on the matrix cores, u rounded to `dtype` on load;
 * a workgroup owns a column block and walks all rows in a fixed order (no atomics: two runs give the same bits). */
int mra_lora_wgrad(const void* x, int64_t ldx, int32_t rows, int32_t N, int32_t dtype, const float* u, int32_t R, float* dw, int32_t dw_layout,
                   float scale, double p, uint64_t seed, void* stream);

/* ---- LM objective: the vocabulary head and its cross-entropy on the labelled rows only -------------------------
 * replaces: lm_head over every position + ForCausalLMLoss inside the reference's self.llm_model(inputs_embeds=..., attention_mask=...,
 * return_dict=True, labels=targets) (models/xinstructblip.py:599-604), of which only the labelled rows matter.  Stateless like mra_lora_*:
 * caller-owned buffers, a stream, no allocation, no synchronisation.  h [R][K] (`dtype` MRA_F16 / MRA_BF16, pitch ldh: the gathered hidden
 * rows after the LM's final norm), W [V][K] (same dtype, pitch ldw: lm_head.weight as stored; never copied, transposed or converted),
 * labels int32 [R].  z = h W^T in fp32, never rounded to 16 bits;  lse_r = log sum_v exp z_rv;  nll_r = lse_r - z_r,y_r;
 * dh_r = g_r (softmax(z_r) - e_y_r) W.  A label outside [0, V) reads nothing out of bounds: that row's nll is NaN (its lse is right) and its
 * dh row is the softmax term g_r softmax(z_r) W alone.
 * Checked before any launch (MRA_EINVAL, named in mra_last_error): negative R, V < 1, K not a positive multiple of 8, unknown dtype, NULL
 * pointers, h / dh / W / workspace not 16-byte aligned, labels / nll / lse / g not 4-byte aligned, a pitch < K or not a multiple of 8, a short
 * workspace.  R == 0 launches nothing, touches nothing and returns MRA_OK whatever else is passed.
 *
 * Workspace bytes, with T = ceil(V / 64) vocabulary tiles, up(x) = x rounded up to 256, and
 * S = ceil(T / ceil(T / min(16, max(1, 512 / (ceil(K / 128) * ceil(R / 128))))))  (integer divisions) splits of the backward's sum over V:
 *     2 up(4 R T) + up(4 R)                       tile maxima, tile sums [R][T] f32, target logits [R] f32
 *   + want_grad ? up(2 R 64 T) + up(4 S R K) : 0  P~ = op(exp(z - tile maximum)) [R][64 T] in `dtype`, partial sums [S][R][K] f32
 * Host only; 0 (and a message) for arguments the entries would refuse. */
size_t mra_lm_head_ce_workspace_bytes(int32_t R, int32_t V, int32_t K, int32_t dtype, int32_t want_grad);
/* One streaming pass over W (a workgroup owns a 64-column vocabulary tile; the ragged tail past V is excluded from maximum and sum) and a merge
 * launch with a fixed order: nll, lse f32 [R].  want_grad != 0 also leaves P~ and the tile maxima in the workspace for the backward; the nll
 * bits do not depend on it. */
int mra_lm_head_ce_forward(const void* h, int64_t ldh, int32_t R, int32_t K, const void* W, int64_t ldw, int32_t V, int32_t dtype,
                           const int32_t* labels, float* nll, float* lse, void* workspace, size_t workspace_bytes, int32_t want_grad, void* stream);
/* dh [R][K] (`dtype`, pitch lddh) = sum_v f_rv P~_rv W_v - g_r W_y_r from the workspace a want_grad forward of the same (R, V, K, W, labels)
 * left; g f32 [R] on the device; the fp32 row factors f = g_r exp(tile maximum - lse_r) are applied inside the product (per tile, to the fp32
 * tile product).  The sum over V is split over S workgroup rows whose fp32 partial sums are added in ascending order, then the one-hot term is
 * subtracted in fp32 and the result rounded once.  No atomics: two runs give the same bits. */
int mra_lm_head_ce_backward(const float* g, const void* W, int64_t ldw, int32_t V, int32_t K, int32_t dtype, const int32_t* labels, const float* lse,
                            void* workspace, size_t workspace_bytes, void* dh, int64_t lddh, int32_t R, void* stream);

/* ---- LM decode: one-token attention over a K/V cache read in place ------------------------------------------------
 * replaces: scaled_dot_product_attention with ONE query row per head inside the reference's self.llm_model.generate(inputs_embeds=...,
 * attention_mask=...) (models/xinstructblip.py:383-391), and with a static cache the torch.cat of a growing one.  Stateless like mra_lora_* and
 * mra_lm_head_ce_*: caller-owned buffers, a stream, no allocation, no synchronisation.  q, out [B][Hq][D], k, v [B][Hkv][S][D] in `dtype`
 * (MRA_F16 / MRA_BF16) with ELEMENT strides (*_sb batch, *_sh head, *_ss key; D contiguous), so a static cache's [B][Hkv][Smax][D] buffer is
 * read as it lies.  mask [B][S] bytes with batch stride mask_sb, nonzero = attend, NULL = every key.  With G = Hq / Hkv:
 *   out[b,h] = softmax_s(scale * q[b,h] . k[b, h / G, s] over the attended s) v[b, h / G]      lse[b,h] = log sum_s exp(scale q.k)  (f32, nullable)
 * Logits, softmax and the P V sum are fp32, P is never rounded to 16 bits, out is rounded once.  A row with no attended key gives out = +0 and
 * lse = -inf.  A masked key is never read: masking is a select, whatever bits the slot holds.
 * A workgroup owns (b, kv head, a chunk of 256 keys) for all G query heads and leaves fp32 partials (m, l, acc[D]) in the workspace; a second
 * launch merges the chunks in ascending order, skipping a chunk without an attended key.  No atomics: two runs give the same bits.
 * Accepted: D 64 or 128, G 1, 2, 4 or 8, S >= 1, B and Hkv at most 65535.  Checked before any launch (MRA_EINVAL, named in mra_last_error):
 * negative B, unknown dtype, another D or G or Hq % Hkv != 0, S < 1, NULL q / k / v / out / workspace, one of them not 16-byte aligned, a
 * stride that is not a multiple of 8 elements, k_ss or v_ss below D, lse not 4-byte aligned, a scale that is not finite, a short workspace.
 * B == 0 launches nothing and returns MRA_OK whatever else is passed.
 *
 * Workspace bytes, with C = ceil(S / 256) chunks and up(x) = x rounded up to 256:   2 up(4 B Hq C) + up(4 B Hq C D)
 * Host only; 0 (and a message) for B < 0, Hq < 1, S < 1 or another D. */
size_t mra_decode_attention_workspace_bytes(int32_t B, int32_t Hq, int32_t S, int32_t D);
int mra_decode_attention(const void* q, int64_t q_sb, int64_t q_sh, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss, const void* v,
                         int64_t v_sb, int64_t v_sh, int64_t v_ss, const uint8_t* mask, int64_t mask_sb, int32_t B, int32_t Hq, int32_t Hkv,
                         int32_t S, int32_t D, int32_t dtype, float scale, void* out, int64_t o_sb, int64_t o_sh, float* lse, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- LM prefill: causal grouped-query attention under a key byte mask -----------------------------------------------
 * replaces: scaled_dot_product_attention under the explicit [Sq][Skv] mask in the prefill inside the reference's
 * self.llm_model.generate(inputs_embeds=..., attention_mask=...) (models/xinstructblip.py:388-391): the first forward over the whole prefix
 * (media rows, timestamps and prompt, left-padded, with padding inside).  Stateless like mra_decode_attention: caller-owned buffers, a stream,
 * no allocation, no synchronisation, no workspace.  q [B][Hq][Sq][D], k, v [B][Hkv][Skv][D] in `dtype` (MRA_F16 / MRA_BF16) with ELEMENT
 * strides (*_sb batch, *_sh head, *_ss position; D contiguous), so a transposed view of q and a static cache's [B][Hkv][Smax][D] buffer are
 * read as they lie.  mask [B][Skv] bytes with batch stride mask_sb, nonzero = attend, NULL = every key; there is no [Sq][Skv] tensor.  Query
 * row i sits at key slot q_offset + i.  out [B][Sq][Hq][D] with element strides o_sb (batch), o_ss (position), o_sh (head); lse f32
 * [B][Hq][Sq] contiguous, natural log, nullable.  With G = Hq / Hkv, for query (b, h, i):
 *   attended = {s : s <= q_offset + i, s < Skv, mask[b][s] != 0}
 *   out = softmax_s(scale * q[b,h,i] . k[b, h / G, s] over the attended s) v[b, h / G]        lse = log sum_s exp(scale q.k)
 * Logits, softmax statistics and the P V sum are fp32 (v_mfma_f32_32x32x16 for both products); P is rounded once to `dtype` for the second
 * product; out is rounded once.  A row with no attended key gives out = +0 and lse = -inf.  Masking is a select on both sides: whatever bits
 * sit in a masked slot, above the diagonal or behind the written part of a static cache reach nothing.
 * A workgroup owns 256 query rows of one (b, query head) and walks tiles of 32 keys, staged once into LDS for its 4 waves, up to the diagonal
 * of its last row; a tile whose mask bytes are all zero is skipped without touching the running maximum or sum; the latest query blocks are
 * launched first.  One launch, no atomics: two runs give the same bits.
 * Accepted: D 64 or 128, G 1, 2, 4 or 8, Sq >= 1, Skv >= 1, 0 <= q_offset, q_offset + Sq <= Skv <= 2^30, B and Hkv at most 65535,
 * Sq at most 65535 * 256.  Checked before the launch (MRA_EINVAL, named in mra_last_error, nothing written): negative B, unknown dtype,
 * another D or G or Hq % Hkv != 0, Sq or Skv < 1, a negative q_offset or q_offset + Sq > Skv, NULL q / k / v / out, one of them not 16-byte
 * aligned, a stride that is not a multiple of 8 elements, q_ss / k_ss / v_ss / o_ss / o_sh below D, lse not 4-byte aligned, a scale that
 * is not finite.  B == 0 launches nothing and returns MRA_OK whatever else is passed. */
int mra_prefill_attention(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                          const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, const uint8_t* mask, int64_t mask_sb, int32_t B, int32_t Hq,
                          int32_t Hkv, int32_t Sq, int32_t Skv, int32_t q_offset, int32_t D, int32_t dtype, float scale, void* out, int64_t o_sb,
                          int64_t o_ss, int64_t o_sh, float* lse, void* stream);

/* ---- LM training: backward of the causal grouped-query attention --------------------------------------------------
 * replaces: the backward of scaled_dot_product_attention under the explicit [S][S] mask inside the reference's
 * self.llm_model(inputs_embeds=..., labels=...) (models/xinstructblip.py:599-604), in every layer of the attached LM.  Stateless like
 * mra_prefill_attention: caller-owned buffers and workspace, a stream, no allocation, no synchronisation, every view by ELEMENT strides (D
 * contiguous).  q and dq are [B][Hq][Sq][D] views (the transposed view of a [B, Sq, Hq, D] tensor works for both), k, v, dk and dv
 * [B][Hkv][Skv][D] views, out and dout [B][Sq][Hq][D] views, mask [B][Skv] bytes or NULL, lse f32 [B][Hq][Sq] as mra_prefill_attention
 * writes it (mandatory).  With att(b, i) = {s : s <= q_offset + i, s < Skv, mask[b][s] != 0} and G = Hq / Hkv:
 *     p_is = exp(scale q[b,h,i] . k[b,h/G,s] - lse_i) on att(b, i), 0 elsewhere and everywhere in a row with lse = -inf
 *     delta_i = dO[b,i,h] . out[b,i,h]            ds_is = p_is (dO[b,i,h] . v[b,h/G,s] - delta_i)
 *     dV[b,g,s] = sum_{h in g} sum_i p_is dO[b,i,h]     dQ[b,h,i] = scale sum_s ds_is k[b,h/G,s]     dK[b,g,s] = scale sum_{h in g} sum_i ds_is q[b,h,i]
 * Logits, p, dp, delta and every sum in fp32 on the MFMAs' accumulators; p and ds are rounded once to `dtype` as MFMA operands, dQ / dK / dV
 * once on the way out.  The sum over a group's query heads runs in registers in ascending head order.  Masking is a select: the bits of a
 * K / V slot that no row attends, and of the dO / out rows of a query row with lse = -inf, reach nothing.  Every element of dq [.., Sq),
 * dk and dv [.., Skv) is written: +0 for a key no row attends and for a row with no attended key.  No atomics: two runs give the same bits.
 * The workspace holds delta, f32 [B][Hq][Sq]; mra_prefill_attention_backward_workspace_bytes gives its size (0 with a reason on bad arguments).
 * Two launches on `stream`.
 * MRA_EINVAL (reason in mra_last_error(), nothing written, before any launch): a negative B, another dtype, D or G, Hq % Hkv != 0, Sq or
 * Skv < 1, a negative q_offset or q_offset + Sq > Skv, a NULL q / k / v / out / dout / lse / dq / dk / dv / workspace, one of the 16-bit
 * buffers or the workspace not 16-byte aligned, lse not 4-byte aligned, a stride that is not a multiple of 8 elements, a position stride (or
 * out's / dout's head stride) below D, a workspace shorter than the size function says, a scale that is not finite.  B == 0 launches nothing
 * and returns MRA_OK whatever else is passed. */
size_t mra_prefill_attention_backward_workspace_bytes(int32_t B, int32_t Hq, int32_t Sq);
int mra_prefill_attention_backward(const void* q, int64_t q_sb, int64_t q_sh, int64_t q_ss, const void* k, int64_t k_sb, int64_t k_sh, int64_t k_ss,
                                   const void* v, int64_t v_sb, int64_t v_sh, int64_t v_ss, const uint8_t* mask, int64_t mask_sb, const void* out,
                                   int64_t o_sb, int64_t o_ss, int64_t o_sh, const void* dout, int64_t do_sb, int64_t do_ss, int64_t do_sh,
                                   const float* lse, int32_t B, int32_t Hq, int32_t Hkv, int32_t Sq, int32_t Skv, int32_t q_offset, int32_t D,
                                   int32_t dtype, float scale, void* dq, int64_t dq_sb, int64_t dq_sh, int64_t dq_ss, void* dk, int64_t dk_sb,
                                   int64_t dk_sh, int64_t dk_ss, void* dv, int64_t dv_sb, int64_t dv_sh, int64_t dv_ss, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* ---- LM decode: one whole token per call (weight-streaming layers, head, greedy bookkeeping) ------------------------
 * replaces: one iteration of the reference's self.llm_model.generate(inputs_embeds=..., attention_mask=..., max_new_tokens=64)
 * (models/xinstructblip.py:383-391, utils/trainer.py:157-165) behind the prefill: the forward of a Llama-shaped LM on one new token per
 * sequence (RMSNorm, q / k / v / o / gate / up / down projections with their optional LoRA branch of models/model_utils.py:4-14, rotary, the
 * cache update, SwiGLU, the residuals, the final norm and lm_head), the argmax and generate's eos / pad bookkeeping.  Stateless like mra_lora_*
 * and mra_decode_attention: caller-owned buffers and workspace, a stream, no allocation, no synchronisation.  1 <= B <= 8 sequences.
 *
 * A linear is W [N][K] in `dtype` (MRA_F16 / MRA_BF16) read as stored with pitch ldw, never copied or transposed, plus an optional adapter:
 * fp32 masters A [R][K] and Bw [N][R] (the layouts mra_lora_* take as MRA_LORA_RN / MRA_LORA_NR), R <= 16 (0: none), scale = alpha / R.
 *   y[b][n] = sum_k x[b][k] W[n][k] + scale * sum_j u[b][j] Bw[n][j],   u[b][j] = sum_k A[j][k] x[b][k]      all fp32, j ascending
 * x is the linear's own input: the normalised rows for q / k / v / gate / up, the attention output for o, the activation for down.  Eval mode:
 * no dropout, nothing is hashed.  Roundings to `dtype`, one each: the residual stream h, q, k, v, the attention output, the SwiGLU activation.
 * Everything inside a launch is fp32: RMSNorm xn = (x * rsqrt(mean(x^2) + eps)) * gain is kept as an fp32 copy and never rounded; the logits
 * are fp32.  Rotary is transformers' Llama rotate-half: x cos + rotate_half(x) sin over the pairs (i, i + D/2), cos / sin fp32 rows
 * [rope_rows][rope_ld] (D values each) indexed by position[b] + pos_offset; a position outside the table writes NaN and reads nothing.
 * k and v of the token go to slot `slot` of the layer's cache [B][Hkv][Smax][D] (ELEMENT strides, as mra_decode_attention takes them), then
 * mra_decode_attention's launch function runs over S = slot + 1 keys under mask [B][>= slot + 1] bytes (the caller has set byte `slot`).
 * Argmax: the first maximum; a NaN counts as the maximum (as torch.argmax), the first NaN wins.  Bookkeeping (finished != NULL): a finished
 * sequence emits pad; a sequence that emits one of the n_eos <= 8 eos ids becomes finished.  tokens_out [B], finished [B] are int32.
 * tokens_in (int32 [B] on the device; NULL: h holds the rows already) selects the embedding rows that start the step; a token outside
 * [0, V) gives a row of NaN.
 *
 * Launches of one call, all plain, in stream order (no atomics, no waits between workgroups; two runs give the same bits):
 *   per token   1 embedding gather (tokens_in != NULL) + 1 final-norm prologue + 1 head + 1 argmax
 *   per layer   8:  norm + u prologue | q / k / v + LoRA + rotary + cache write | attention chunks | attention merge | o + residual |
 *                   norm + u prologue | gate / up + SwiGLU | down + residual;  + 1 for an adapter on o, + 1 for one on down (their u = A x)
 * Refused before any launch (MRA_EINVAL, named in mra_last_error): struct_bytes != sizeof, B outside 1..8, hidden / intermediate not positive
 * multiples of 8, D outside {64, 128}, Hq / Hkv outside {1, 2, 4, 8}, L < 1, V < 1, an unknown dtype, R outside 0..16, an N that is not the
 * layer's, slot outside [0, Smax), a NULL or misaligned (16 bytes; int32 / fp32 vectors 4) buffer, a pitch or stride that is short or not a
 * multiple of 8 elements, a short workspace, eps or attn_scale not finite, n_eos outside 0..8.
 *
 * Workspace bytes, up(x) = x rounded up to 256:  up(4 B hidden) + 3 up(64 B) + 2 up(2 B Hq D) + up(2 B intermediate)
 *                                               + mra_decode_attention_workspace_bytes(B, Hq, Smax, D).   Host only; 0 (and a message) when refused. */
typedef struct mra_lm_linear {
  const void* W;   /* [N][K] dtype */
  int64_t ldw;
  const float* A;  /* [R][K] fp32, NULL when R == 0 */
  const float* Bw; /* [N][R] fp32 */
  int32_t N;
  int32_t R;
  float scale;
  int32_t reserved;
} mra_lm_linear;
typedef struct mra_lm_layer {
  const void* norm1; /* input_layernorm.weight [hidden] dtype */
  const void* norm2; /* post_attention_layernorm.weight */
  mra_lm_linear q, k, v, o, gate, up, down;
  void* kcache; /* [B][Hkv][Smax][D] dtype, strides below */
  void* vcache;
} mra_lm_layer;
typedef struct mra_lm_step_desc {
  uint64_t struct_bytes;
  int32_t B, hidden, intermediate, Hq, Hkv, D, L, V, dtype, Smax;
  float eps, attn_scale;
  const mra_lm_layer* layers; /* HOST array of L records */
  const void* embed;          /* [V][hidden] dtype */
  int64_t ld_embed;
  const void* final_norm;
  const void* head;           /* lm_head.weight [V][hidden] dtype */
  int64_t ld_head;
  int64_t k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;
  const uint8_t* mask;
  int64_t mask_sb;
  const int32_t* position;
  int32_t pos_offset, slot;
  const float* cos;
  const float* sin;
  int64_t rope_ld;
  int32_t rope_rows, n_eos;
  const int32_t* tokens_in;
  void* h;                    /* [B][hidden] dtype, dense: the residual stream; holds the final hidden rows afterwards */
  float* logits;              /* [B][ld_logits >= V] fp32 */
  int64_t ld_logits;
  int32_t* tokens_out;
  int32_t* finished;          /* may be NULL */
  int32_t pad;
  int32_t eos[8];
  int32_t reserved;
  void* workspace;
  uint64_t workspace_bytes;
} mra_lm_step_desc;
size_t mra_lm_step_workspace_bytes(int32_t B, int32_t hidden, int32_t intermediate, int32_t Hq, int32_t D, int32_t Smax);
int mra_lm_step(const mra_lm_step_desc* desc, void* stream);

/* mra_debug_lm_skinny: ONE launch of the step's skinny kernel in any of its forms (behind its prologue launch when norm_gain or an adapter is
 * given), as mra_lm_step issues it.  epilogue 0 plain (out_f32 != 0: fp32 output) | 1 + residual | 2 SwiGLU (seg 0 gate, seg 1 up, out[0]) |
 * 3 rotary + cache write (seg 0 / 1 / 2 = q / k / v with N = Hq D, Hkv D, Hkv D; q to out[0]).  nseg 1..3 segments share x [B][K] (pitch ldx).
 * Every buffer comes with its byte size; checked on the host before the launch (MRA_EINVAL with a message): struct_bytes, the refusals of
 * mra_lm_step that apply, every pointer NULL / misaligned, every pitch below its width or not a multiple of 8 elements (fp32: 4), every
 * footprint ((rows - 1) pitch + width elements; a cache: through slot `slot` of the last head of the last row) beyond its byte size.
 * workspace: up(4 B K) + 3 up(64 B) bytes. */
typedef struct mra_lm_skinny_desc {
  uint64_t struct_bytes;
  int32_t B, K, dtype, epilogue, nseg, out_f32;
  const void* x;
  int64_t ldx;
  uint64_t x_bytes;
  const void* norm_gain; /* [K] dtype; NULL: no RMSNorm prologue */
  float eps;
  int32_t reserved;
  mra_lm_linear seg[3];
  uint64_t w_bytes[3];
  void* out[3];
  int64_t ldo[3];
  uint64_t out_bytes[3];
  const void* res;
  int64_t ldres;
  uint64_t res_bytes;
  int32_t Hq, Hkv, D, slot, pos_offset, rope_rows;
  const int32_t* position;
  const float* cos;
  const float* sin;
  int64_t rope_ld;
  uint64_t rope_bytes;
  void* kcache;
  void* vcache;
  int64_t k_sb, k_sh, k_ss, v_sb, v_sh, v_ss;
  uint64_t kcache_bytes, vcache_bytes;
  void* workspace;
  uint64_t workspace_bytes;
} mra_lm_skinny_desc;
int mra_debug_lm_skinny(const mra_lm_skinny_desc* desc, void* stream);
/* mra_debug_lm_argmax: the step's argmax + bookkeeping launch alone.  logits fp32 [B][ld >= V]; eos HOST array of n_eos <= 8 ids. */
int mra_debug_lm_argmax(const float* logits, int64_t ld, int32_t B, int32_t V, int32_t* tokens_out, int32_t* finished, int32_t pad,
                        const int32_t* eos, int32_t n_eos, void* stream);

/* ---- LM objective: prompt assembly as one row gather -------------------------------------------------------------
 * replaces: the torch.cat of cue, media, timestamp, duration and prompt pieces in front of the LM (models/xinstructblip.py:341-381, :541-595)
 * and, through the inverse plan, its backward.  Stateless like mra_lora_* and mra_lm_head_ce_*: caller-owned buffers, a stream, no allocation,
 * no synchronisation.  out [n_rows][width] (out_dtype, pitch ldo);  plan int32 [n_rows][2] = (source, row) on the DEVICE;  srcs a HOST array.
 *   out[i][0:width] = cast(srcs[s].ptr[r * srcs[s].ld + 0:width])   for plan[i] = (s, r), 0 <= s < n_src, 0 <= r < srcs[s].rows
 *   s == -1 writes a row of +0;  every other entry out of range reads nothing and writes a row of NaN (as a bad label does in mra_lm_head_ce_*).
 * Casts: f32 -> f16 / bf16 rounds to nearest even (overflow to infinity, NaN stays NaN); f16 / bf16 -> f32 is exact; equal types are a bit
 * copy; f16 <-> bf16 is refused.  The backward of a gather whose rows are used at most once is the same entry with d_out as the one source and
 * the inverse plan.  A wave owns an output row: no atomics, two runs give the same bits.
 * Checked before any launch (MRA_EINVAL, named in mra_last_error): negative n_rows, NULL out / srcs / plan / a source's ptr, n_src outside 1..4,
 * width not a positive multiple of 8, an unknown dtype or a refused pair, negative source rows, a pitch below width or not a multiple of 16
 * bytes, out or a source not 16-byte aligned, plan not 8-byte aligned.  n_rows == 0 launches nothing and returns MRA_OK whatever else is passed. */
typedef struct mra_rows_src {
  const void* ptr; /* device, [rows][ld] of dtype */
  int64_t ld;      /* pitch in elements */
  int32_t rows;
  int32_t dtype;   /* MRA_F32 / MRA_F16 / MRA_BF16 */
} mra_rows_src;
int mra_gather_rows(void* out, int64_t ldo, int32_t out_dtype, int32_t n_rows, int32_t width, const mra_rows_src* srcs, int32_t n_src,
                    const int32_t* plan, void* stream);

/* ---- A6: scorer (build-defined; the reference has no scorer) ----------------------------------
 * sim[n][q] = cos(z[n][q][:], t[n or 0][:]); logit[n] = max_q sim[n][q].  sim may be NULL. */
int mra_cosine_score(const float* z, const float* t, int32_t t_rows, int32_t items, int32_t n_query, int32_t hidden,
                     float* sim, float* logit, void* stream);
/* out[i] = sum_m weights[m] * logits[m][i] (weights NULL = 1/nmod), fp32, left to right. */
int mra_fuse_logits(const float* const* logits, const float* weights, int32_t nmod, int32_t n, float* out,
                    void* stream);
/* spans[v] = (start, end) inclusive clip indices grown around the first argmax of
 * logits[v*clips .. (v+1)*clips) while the neighbour >= lo + alpha * (hi - lo). */
int mra_span_from_logits(const float* logits, int32_t videos, int32_t clips, float alpha, int32_t* spans,
                         void* stream);
/* Ranked moment proposals: per video the top_k windows of its fused clip logits under greedy temporal NMS.
 * replaces: the ranked pred_relevant_windows list that eval/mr_eval.py:21-94 consumes in list order and that the
 * reference's LLM decode could emit as "[[a, b], [c, d]]" (utils/utils.py:66-132).  Build-defined like the rest of
 * A6 (the reference has no scorer); a second head beside mra_span_from_logits, which is unchanged.
 * Definition, per video with x = logits[v*clips .. (v+1)*clips), finite:
 *   1. hi = max x, lo = min x, thr = lo + alpha * (hi - lo) in fp32, product and sum rounded separately
 *      (as mra_span_from_logits);
 *   2. q[i] = llrint(clamp((double)x[i] * 2^20, +-2^40)) - llrint(clamp((double)thr * 2^20, +-2^40))  (int64);
 *   3. P[0] = 0, P[i+1] = P[i] + q[i]  (exact);
 *   4. candidates: every (s, e), 0 <= s <= e < clips, inclusive clip indices, with e - s + 1 <= max_len
 *      (max_len == 0: no cap); score(s, e) = P[e+1] - P[s], the summed excess over the threshold;
 *   5. order: higher score, then the shorter window, then the smaller s;
 *   6. greedy NMS in that order: a candidate is dropped when for a selected window (s', e')
 *      (double)inter > (double)nms_thd * (double)union, inter = max(0, min(e, e') - max(s, s') + 1),
 *      union = len + len' - inter (the product is exact; nms_thd < 1 always drops an identical window);
 *   7. rank 1 is always emitted (its score is >= 0: the argmax clip alone qualifies); later ranks only while the best
 *      remaining score is > 0; at most top_k.
 * Rank 1 is a maximum-sum window; it need not equal the span of mra_span_from_logits (it may bridge a short dip).
 * windows [videos, top_k, 2] int32 (unused slots -1), scores [videos, top_k] = (float)((double)score * 2^-20)
 * (unused slots 0), counts [videos].  clips in 1..4096, top_k in 1..64, nms_thd in [0, 1), max_len >= 0.
 * One launch, no allocation, no synchronisation.  For non-finite logits the results are unspecified (the kernel
 * still terminates in bounds).  Cost grows with clips^2 when max_len == 0: see DESIGN.md section 4. */
int mra_windows_from_logits(const float* logits, int32_t videos, int32_t clips, float alpha, int32_t top_k,
                            float nms_thd, int32_t max_len, int32_t* windows, float* scores, int32_t* counts,
                            void* stream);

/* ---- training: forward with an activation tape + backward (BASELINE config 5) --------------------
 * Beyond the reference: its Q-Formers are frozen (models/xinstructblip.py:196-204) and utils/trainer.py
 * only updates LoRA adapters of the LLM; the north star asks for a Q-Former fwd+bwd step.  Checked
 * against torch.autograd over the CPU oracle.
 *   mra_qformer_enable_training   builds the transposed weight copies the data-gradient GEMMs read
 *                                 (allocates once; call again after every weight upload)
 *   mra_qformer_forward_train     as mra_qformer_forward (loaded query tokens, optional out_cls) but
 *                                 every layer keeps its activations in `workspace`, which must stay
 *                                 untouched until the matching mra_qformer_backward
 *   mra_qformer_backward          d_out_query [items, n_query, hidden] and/or d_out_cls [items, hidden]
 *                                 (f32, NULL = zero) -> ADDS parameter gradients into `grads`, a flat f32
 *                                 buffer of mra_qformer_grad_bytes() in which parameter `name` (same names
 *                                 as mra_qformer_load) owns numel floats at mra_qformer_grad_offset().
 *                                 Gradients flow to every Q-Former parameter incl. query_tokens and the
 *                                 embeddings; enc and ln.* get theirs from mra_qformer_backward_enc and
 *                                 mra_modality_ln_backward (below); llm_proj.* is not on the scorer's path
 *                                 (its gradients come from mra_llm_proj_backward, never into `grads`). */
size_t mra_qformer_grad_bytes(mra_qformer* h);
/* Optimizer-side fast path: refreshes EVERY bert.* parameter in one launch from a flat f32 master buffer
 * laid out exactly like the gradient buffer (parameter `name` at mra_qformer_grad_offset(name)), converting
 * matrices to the operand dtype on the way.  An optimizer that keeps its master weights in that layout
 * (mraudio_amd.qformer re-points every nn.Parameter at its slice) pays one ~0.3 ms kernel per step instead of
 * ~400 mra_qformer_load calls.  query_tokens / ln.* / llm_proj.* still go through mra_qformer_load.
 * No counterpart in the reference (DDP + torch.optim over autograd parameters, utils/trainer.py:60-69). */
int32_t mra_qformer_load_flat(mra_qformer* h, const float* master, size_t master_bytes, void* stream);
int mra_qformer_grad_offset(mra_qformer* h, const char* name, size_t* offset_bytes, int64_t* numel);
int mra_qformer_enable_training(mra_qformer* h, void* stream);
/* The optimizer step of BASELINE config 5 in ONE pass over the flat buffers (replaces, on the hot path, torch.optim.Adam's
 * multi_tensor_apply + mra_qformer_load_flat + the transposed-copy rebuild; caller: utils/trainer.py:137-140 `scaler.step(optimizer)`):
 * torch.optim.Adam's arithmetic (L2 weight decay added to the gradient, bias correction from `step` >= 1) on master / grad / exp_avg /
 * exp_avg_sq -- four fp32 buffers of mra_qformer_grad_bytes() in the gradient buffer's layout -- and, from the same registers, every device
 * copy the update makes stale: the operand-dtype weights, their transposed training copies, fp32 biases / LayerNorms / embeddings / query
 * tokens.  zero_grad != 0 clears the gradient buffer on the way.  ~30 B per parameter of HBM traffic instead of ~50. */
int mra_qformer_adam_step(mra_qformer* h, float* master, float* grad, float* exp_avg, float* exp_avg_sq, size_t bytes, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int32_t step, int32_t zero_grad, void* stream);
size_t mra_qformer_train_workspace_bytes(mra_qformer* h, int32_t items, int32_t L, int32_t kv);
int mra_qformer_forward_train(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask, const void* enc,
                              int32_t items, int32_t L, int32_t kv, float* out_query, float* out_cls, void* workspace,
                              size_t workspace_bytes, void* stream);
int mra_qformer_backward(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask, const void* enc,
                         int32_t items, int32_t L, int32_t kv, const float* d_out_query, const float* d_out_cls,
                         float* grads, void* workspace, size_t workspace_bytes, void* stream);

/* Multi-query training step: `prompts` chain items per encoder item over ONE K/V cache, forward with a tape and backward.  Defined as one
 * mra_qformer_forward_train / mra_qformer_backward pair on enc repeated `prompts` times per item (row i * prompts + p reads encoder item i),
 * without the repetition:
 *   input_ids      [enc_items * prompts, L]       int64   row i * prompts + p: encoder item i, prompt slot p; prompts differ freely per row
 *   attention_mask [enc_items * prompts, 32 + L]  int64   same row order, or NULL (all ones)
 *   enc            [enc_items, kv, E]             operand dtype, as mra_modality_ln writes it
 *   out_query / d_out_query  [enc_items * prompts, 32, H]  fp32 (may be NULL)
 *   out_cls / d_out_cls      [enc_items * prompts, H]      fp32 (may be NULL; needs L >= 1)
 * The layer chain, its tape and its gradients run on enc_items * prompts items.  The K/V projection, the K/V cache, the dK / dV tape and
 * the dW_k / dW_v weight gradients run on enc_items items: per cross layer and encoder item the projection and its weight gradient cost
 * 4 Kv E 768 flops each (call it 1 each) -- 2 per encoder item here, 2 prompts on a repeated enc (arithmetic, not a measurement).  dK / dV
 * of an encoder item are summed over its prompts in registers inside the attention backward, rounded once; no atomics.
 * The cross core of the tape forward is the core of mra_qformer_forward_train with each chain item taking the K/V of item n / prompts, and
 * writes the log-sum-exp the backward needs, whatever mra_qformer_set_option "multi_core" says: the shared-stream core writes none and is
 * not used here.  Long KV splits by the rule of mra_qformer_forward_train on chain items.  Precision as mra_qformer_forward_train.
 * Argument checks worded as mra_qformer_forward_multi (prompts >= 1, enc_items == 0 is a no-op); ownership, workspace lifetime and
 * ADD-into-grads as mra_qformer_forward_train / mra_qformer_backward, which ARE these entries at prompts = 1, launch for launch, behind what
 * their older contract keeps: items <= 0 or kv <= 0 is MRA_EINVAL; the forward reports a misaligned workspace as MRA_ENOMEM and runs with
 * neither output asked for.  mra_qformer_backward thereby refuses with MRA_EINVAL what it used to launch on: L above max_pos, NULL input_ids
 * with L > 0, d_out_cls with L < 1.  The attention backward keeps fp32 dQ / lse / delta of all prompts of an encoder item in LDS: prompts
 * above 14 (at 32 query rows, 160 KB) -> MRA_EINVAL naming the limit; split the group.  Workspace: mra_qformer_multi_train_workspace_bytes
 * (0 for a NULL handle or a non-positive size), 256-byte aligned. */
size_t mra_qformer_multi_train_workspace_bytes(mra_qformer* h, int32_t enc_items, int32_t prompts, int32_t L, int32_t kv);
int mra_qformer_forward_multi_train(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask, const void* enc,
                                    int32_t enc_items, int32_t prompts, int32_t L, int32_t kv, float* out_query, float* out_cls,
                                    void* workspace, size_t workspace_bytes, void* stream);
int mra_qformer_backward_multi(mra_qformer* h, const int64_t* input_ids, const int64_t* attention_mask, const void* enc,
                               int32_t enc_items, int32_t prompts, int32_t L, int32_t kv, const float* d_out_query, const float* d_out_cls,
                               float* grads, void* workspace, size_t workspace_bytes, void* stream);

/* Encoder side of the training step: gradients to the features the Q-Former was fed and to the modality LayerNorm in front of it.  Nothing
 * here runs unless it is called.
 * mra_qformer_backward_enc: after the matching backward (mra_qformer_backward: prompts = 1), on the untouched tape.  The
 *   backward leaves dK / dV of every cross layer in the workspace (head-major [ncross][k | v][enc_items][heads][kv][64], operand dtype, for a
 *   multi call already summed over the prompts of an item); this call contracts them with the stored K / V weights,
 *     d_enc[item * kv + tok][e] = sum_k dKV[item * kv + tok][k] W_kv[k][e],   k = (cross layer * 2 + k | v) * hidden + head * 64 + d,
 *   reading the cache in place (no token-major copy) and the weights as stored (no transposed copy): one launch, MFMA with fp32 accumulation,
 *   the flops of one mra_kv_project.  d_enc [enc_items, kv, E] fp32 is WRITTEN: the gradient with respect to the operand-dtype enc given to
 *   the forward (the rounding to the operand dtype is passed straight through, like every 16-bit tensor of the tape).  enc_width must be a
 *   multiple of 128.  Checks as the training entries: prompts >= 1, negative size, NULL workspace / d_enc / handle (MRA_EINVAL); training not
 *   enabled or the transposed copies stale (MRA_ESTATE); workspace_bytes below mra_qformer_multi_train_workspace_bytes(h, enc_items,
 *   prompts, L, kv) (MRA_ENOMEM).  enc_items == 0 is a no-op.  No allocation,
 *   no synchronisation.
 * mra_modality_ln_backward: backward of mra_modality_ln without an item index, with the handle's loaded ln.weight and enc_ln_eps (MRA_ESTATE
 *   if ln.* is not loaded).  x [items, tokens, E] is the raw feature tensor the forward read (MRA_F32 / MRA_F16 / MRA_BF16), d_out [items,
 *   tokens, E] fp32 the upstream gradient (mra_qformer_backward_enc's d_enc).  Statistics are recomputed two-pass from x:
 *     d_x = r (g - mean(g) - xhat mean(g xhat)), g = d_out gain;   d_gain += sum_rows d_out xhat;   d_bias += sum_rows d_out.
 *   d_x [items, tokens, E] fp32 is written and may be d_out itself (a row is read completely before it is written); d_gain / d_bias [E] fp32
 *   are ADDED to (float atomics: the order over rows is not fixed).  Any of d_x, d_gain, d_bias may be NULL.  One launch, no allocation.
 * mra_debug_kvgrad_gemm: the GEMM of mra_qformer_backward_enc alone on a caller-supplied cache dkv [ncross * 2][enc_items][heads][kv][64]
 *   (operand dtype, 16-byte aligned) with the handle's K / V weights; needs neither a tape nor enabled training.  The read and the write
 *   footprint are checked on the host against dkv_bytes and d_enc_bytes before the launch. */
int mra_qformer_backward_enc(mra_qformer* h, int32_t enc_items, int32_t prompts, int32_t L, int32_t kv, const void* workspace,
                             size_t workspace_bytes, float* d_enc, void* stream);
int mra_modality_ln_backward(mra_qformer* h, const void* x, int32_t x_dtype, int32_t items, int32_t tokens, const float* d_out, float* d_x,
                             float* d_gain, float* d_bias, void* stream);
int mra_debug_kvgrad_gemm(mra_qformer* h, const void* dkv, size_t dkv_bytes, int32_t enc_items, int32_t kv, float* d_enc, size_t d_enc_bytes,
                          void* stream);

/* ---- introspection for the bench ------------------------------------------------------------------
 * Algorithmic flop count of one mra_qformer_forward (2 flops per MAC; formula in DESIGN.md). */
double mra_qformer_flops(mra_qformer* h, int32_t items, int32_t L, int32_t kv, int32_t with_last_text);

/* ---- EVA ViT-g/14 visual encoder (row A1 / N4) -----------------------------------------------------------
 * replaces: self.video_encoder(frame) inside the per-position loop of XInstructBLIP.generate / forward
 * (models/xinstructblip.py:262-266, :412-420), the module create_eva_vit_g(224, 0, False, "fp16") builds (:658-666).
 * One call encodes ALL frames of a step (the reference's T sequential calls at batch B, collapsed).  Parameter names are
 * the state_dict keys of mraudio_amd/models/eva_vit.py (cls_token, pos_embed, patch_embed.{weight,bias},
 * blocks.{i}.{norm1,norm2}.{weight,bias}, blocks.{i}.attn.{qkv.weight,q_bias,v_bias,proj.weight,proj.bias},
 * blocks.{i}.{fc1,fc2}.{weight,bias}); EvaViTg.hf_state_dict / load_hf_state_dict map them to the HF vision tower. */
typedef struct mra_vit mra_vit;
typedef struct mra_vit_cfg {
  int32_t dim;       /* 1408; multiple of 176 and 64 */
  int32_t heads;     /* 16; head dimension dim / heads = 88 (<= 96, multiple of 8) */
  int32_t mlp;       /* 6144 */
  int32_t depth;     /* 39 (LAVIS drops the 40th EVA block) */
  int32_t patch;     /* 14 */
  int32_t img;       /* 224 -> (224 / 14)^2 + 1 = 257 tokens */
  float ln_eps;      /* 1e-6 */
  int32_t op_dtype;  /* MRA_F16 (the reference's precision="fp16") or MRA_BF16: MFMA operand type */
  int32_t residual_dtype;  /* MRA_F32 (default: fp32 residual stream, the accurate choice) or the operand dtype (the reference's own
                            * precision="fp16" semantics: every residual add rounds to 16 bits; half the epilogue and LayerNorm bytes) */
} mra_vit_cfg;
void mra_vit_cfg_default(mra_vit_cfg* cfg);
int mra_vit_create(const mra_vit_cfg* cfg, mra_vit** out);
void mra_vit_destroy(mra_vit* h);
int mra_vit_load(mra_vit* h, const char* name, const void* src, int32_t dtype, const int64_t* shape, int32_t ndim, void* stream);
/* number of parameters not loaded yet (0 = ready) */
int mra_vit_missing(mra_vit* h);
size_t mra_vit_workspace_bytes(mra_vit* h, int32_t frames);
/* frames [n, 3, img, img] (MRA_F32 or MRA_F16, normalised pixels) -> out [n, tokens, dim] in cfg.residual_dtype: the last block's
 * output, no final norm (the reference's separate video_ln, mra_modality_ln, consumes it in place). */
int mra_vit_forward(mra_vit* h, const void* frames, int32_t dtype, int32_t n, void* out, void* workspace, size_t workspace_bytes,
                    void* stream);
/* algorithmic flops of one forward over `frames` frames (2 per MAC) */
double mra_vit_flops(mra_vit* h, int32_t frames);
/* Per-handle options.  "ln_fold" (default 1; dim = 256 k + 128 only, otherwise ignored): the two LayerNorms of a
 * block (HF modeling_instructblip.py:392-440 layer_norm1 / layer_norm2, the callee of /root/reference/models/xinstructblip.py:262-266) are folded
 * into the GEMMs around them -- LN(x) W^T + b = rstd (x (W diag(g))^T - mu colsum(W diag(g))) + (b + W beta): the residual GEMM before a
 * LayerNorm also writes the rows' operand-dtype copy and 128-column statistics (with the residual stream in the operand dtype the stream is
 * that copy and only 64-column statistics are added), the QKV / fc1 GEMM finishes the LayerNorm in its epilogue; the rows are not read back and
 * no LayerNorm kernel runs.  0: separate LayerNorm launches (round 2's form), for A/B and parity runs.
 * "gemm_persist" (default 1): the QKV / fc1 GEMMs as ONE persistent workgroup per CU walking over the output tiles in the launch's tile order
 * instead of one workgroup per tile (no workgroup turnaround, arguments fetched once; bit-identical results; 0 = off, 2 = only up to 64 rounds).
 * "attn_persist" (default 0; 257-token frames): 1 = the attention core as one persistent workgroup per CU that fetches the K / V rows of its
 * next (frame, head) unit into registers while it works on the current one (bit-identical results; measured slower). */
int mra_vit_set_option(mra_vit* h, const char* name, int32_t value);

/* ---- BEATs audio encoder (row A1 / N4, the audio half) ----------------------------------------------------
 * replaces: self.audio_encoder(fbank) inside the per-position loop of XInstructBLIP.generate / forward
 * (models/xinstructblip.py:267-275), the module LAVIS BeatsEncoder(checkpoint_path) builds (init_audio_encoder, :670-676), whose
 * forward is BEATs' extract_features(fbank, padding_mask=None, feature_only=True)[0].
 * One call encodes ALL clip chunks of a step.  Parameter names are the state_dict keys of mraudio_amd/models/beats.py, which are
 * BEATs' checkpoint keys (patch_embedding.weight, layer_norm.{weight,bias}, post_extract_proj.{weight,bias},
 * encoder.pos_conv.0.{weight,bias}, encoder.layer_norm.{weight,bias},
 * encoder.layers.{i}.self_attn.{q_proj,k_proj,v_proj,out_proj,grep_linear}.{weight,bias}, encoder.layers.{i}.self_attn.grep_a,
 * encoder.layers.0.self_attn.relative_attention_bias.weight, encoder.layers.{i}.{self_attn_layer_norm,fc1,fc2,final_layer_norm}.{weight,bias})
 * with one exception: the positional convolution is loaded as its EFFECTIVE weight "encoder.pos_conv.0.weight" [dim, dim / groups, conv_pos]
 * (weight_g * weight_v / ||weight_v||, folded by the caller: the encoder is frozen).  k_proj.bias is optional (zero when not loaded).
 * BEATs.hf_state_dict / load_hf_state_dict map the transformer part to transformers' WavLMEncoder. */
#define MRA_BEATS_GATE_Q 0      /* BEATs: the gate of the relative-position bias is computed from the unscaled q projection */
#define MRA_BEATS_GATE_INPUT 1  /* WavLM: from the layer input */
typedef struct mra_beats mra_beats;
typedef struct mra_beats_cfg {
  int32_t dim;              /* encoder_embed_dim 768; heads * 64, multiple of 256 */
  int32_t heads;            /* encoder_attention_heads 12 (head dimension 64) */
  int32_t ffn;              /* encoder_ffn_embed_dim 3072; multiple of 256 */
  int32_t layers;           /* encoder_layers 12 */
  int32_t embed_dim;        /* patch embedding width 512; multiple of 256 */
  int32_t patch;            /* input_patch_size 16 */
  int32_t mel_bins;         /* 128 -> mel_bins / patch = 8 tokens per patch row */
  int32_t conv_pos;         /* 128 taps of the positional convolution (even) */
  int32_t conv_pos_groups;  /* 16: dim / groups = 48 channels per group */
  int32_t num_buckets;      /* 320 relative-position buckets */
  int32_t max_distance;     /* 800 */
  float ln_eps;             /* 1e-5 */
  float deep_norm_alpha;    /* residual scale of the post-LN layers: (2 * layers)^0.25 for BEATs, 1 for WavLM */
  int32_t gate_from;        /* MRA_BEATS_GATE_Q (BEATs) or MRA_BEATS_GATE_INPUT (WavLM) */
  int32_t op_dtype;         /* MRA_F16: MFMA operand type (the reference autocasts the encoders to fp16) */
} mra_beats_cfg;
void mra_beats_cfg_default(mra_beats_cfg* cfg);
int mra_beats_create(const mra_beats_cfg* cfg, mra_beats** out);
void mra_beats_destroy(mra_beats* h);
int mra_beats_load(mra_beats* h, const char* name, const void* src, int32_t dtype, const int64_t* shape, int32_t ndim, void* stream);
/* number of required parameters not loaded yet (0 = ready) */
int mra_beats_missing(mra_beats* h);
size_t mra_beats_workspace_bytes(mra_beats* h, int32_t n, int32_t frames);
/* fbank [n, frames, mel_bins] (MRA_F32 or MRA_F16, the normalised filterbank BeatsAudioProcessor emits; frames are truncated to a
 * multiple of patch) -> out [n, P, dim] fp32 with P = frames / patch * mel_bins / patch tokens (<= 512): the last layer's output. */
int mra_beats_forward(mra_beats* h, const void* fbank, int32_t dtype, int32_t n, int32_t frames, void* out, void* workspace,
                      size_t workspace_bytes, void* stream);
/* executed flops of one forward over n chunks of `frames` frames (2 per MAC) */
double mra_beats_flops(mra_beats* h, int32_t n, int32_t frames);
/* Per-handle options.  "gemm_persist" (default 1): the QKV / fc1 GEMMs as one persistent workgroup per CU (as mra_vit_set_option). */
int mra_beats_set_option(mra_beats* h, const char* name, int32_t value);

/* ---- audio front end: waveform -> normalised filterbank (row A1, the input side of the audio half) ------------------
 * replaces: LAVIS BeatsAudioProcessor.__call__ -> torchaudio.compliance.kaldi.fbank (call sites evaluate.py:24,
 * utils/trainer.py:46), the host-side producer of the [T, frame_length, 128] tensors mra_beats_forward consumes.  The arithmetic
 * is that of mraudio_amd/processors/audio_processors.py (kaldi_fbank with BEATs' arguments, then (x - 15.41663) / (2 * 6.55582));
 * those arguments are constants of the kernel, so there is no configuration struct.  fp32 throughout.
 * mra_fbank_create builds the window / transform / mel tables on the host in float64 and uploads them: the only allocation. */
typedef struct mra_fbank mra_fbank;
int mra_fbank_create(mra_fbank** out);
void mra_fbank_destroy(mra_fbank* h);
/* wave fp32 [total_samples] (device; mono, 16 kHz, in [-1, 1]); segs int64 [n_seg][2] (device): first sample and number of
 * samples of each temporal position, clipped to [0, total_samples) inside the kernel; out [n_seg, frame_length, 128] (device,
 * MRA_F32 or MRA_F16): frame t of a segment is its 400 samples at 160 t (snip_edges), rows past its last frame are written as
 * zero.  One launch; no allocation, no synchronisation, no host read of segs.  n_seg == 0 is a no-op. */
int mra_fbank_forward(mra_fbank* h, const float* wave, int64_t total_samples, const int64_t* segs, int32_t n_seg, int32_t frame_length,
                      void* out, int32_t out_dtype, void* stream);
/* executed flops of one forward (2 per MAC: the dense 400 x 512 transform, the power spectrum, the sparse mel sums) */
double mra_fbank_flops(mra_fbank* h, int32_t n_seg, int32_t frame_length);

/* ---- audio front end: band-limited resampling to the model's rate (row A1, in front of mra_fbank_forward) ------------
 * replaces: the resampling inside LAVIS BeatsAudioProcessor.__call__ (torchaudio's windowed-sinc `resample`: Hann window,
 * lowpass_filter_width 6, rolloff 0.99), with the channel downmix.  The arithmetic is that of
 * mraudio_amd/processors/audio_processors.py (resample_sinc, the definition; resample_table, the sparse per-phase form the kernel
 * uses); those arguments are constants.  fp32 throughout.  With g = gcd(rate_in, rate_out), orig = rate_in / g, new = rate_out / g.
 * mra_resample_create builds the per-phase tap table on the host in float64, rounds it to fp32 once and uploads it: the only
 * allocation.  Arguments are checked before anything touches the GPU; MRA_EINVAL with a message naming the limit for a rate <= 0, a
 * NULL out, and a rate pair beyond the kernel's limits: new <= 1024 phases, <= 256 taps per phase (2 * 6 * orig / (0.99 min(orig,
 * new)) + 1), a table new * (taps | 1) <= 16384 coefficients, and ceil(1023 * orig / new) + taps + 1 <= 16384 staged input samples
 * per workgroup.  Every pair of {8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000} -> 16000 is admitted;
 * equal rates give the identity (the channel mean). */
typedef struct mra_resample mra_resample;
int mra_resample_create(int32_t rate_in, int32_t rate_out, mra_resample** out);
void mra_resample_destroy(mra_resample* h);
/* ceil(new * n_in / orig): the output length of a clip of n_in samples per channel.  No handle, no GPU; 0 for a rate <= 0 or n_in < 0. */
int64_t mra_resample_out_samples(int32_t rate_in, int32_t rate_out, int64_t n_in);
/* wave fp32 [total_in] (device): the clips of a step that share rate_in, concatenated; clips int64 [n_clip][6] (device), per clip
 *   {first input sample, samples per channel n_in, channels C (planes consecutive: channel c at first + c * n_in; 1 .. 32),
 *    first output sample, output samples n_out, first workgroup}
 * with first workgroup = the sum of ceil(n_out / 1024) over the rows before (ascending); out fp32 [total_out] (device): output m of
 * a clip, the filter over the channel MEAN of its samples with zeros outside [0, n_in), goes to first output sample + m.  A clip's
 * output does not depend on its neighbours in the buffer.  One launch of total_out / 1024 + n_clip workgroups (the outputs of the
 * clips are disjoint parts of out, so this covers every row); the host side does not read the table, allocates nothing and does
 * not synchronise.  Inside the kernel every row is clipped: no read outside [0, total_in), no write outside [0, total_out).
 * n_clip == 0 (or total_out == 0) is a no-op. */
int mra_resample_forward(mra_resample* h, const float* wave, int64_t total_in, const int64_t* clips, int32_t n_clip, float* out,
                         int64_t total_out, void* stream);
/* executed flops of total_out output samples (2 per MAC over the non-zero taps, averaged over the phases) */
double mra_resample_flops(mra_resample* h, int64_t total_out);

/* ---- video front end: decoded uint8 frames -> the encoder's normalised pixels (row A1, in front of mra_vit_forward) ------------
 * replaces: LAVIS AlproVideoTrainProcessor.transform / AlproVideoEvalProcessor.transform on the host (random resized crop of the whole
 * clip, bicubic; horizontal flip; ToUint8; / 255; Normalize) and the host permutes to [B*T, 3, H, W].  The arithmetic is that of
 * mraudio_amd/processors/alpro_processors.py (crop_resize_table and preprocess_frames_ref, the float64 definition, pinned there to
 * torch's bicubic interpolate with align_corners = False): separable 4-tap tables with cubic coefficient A = -0.75, source coordinate
 * (crop / out)(o + 0.5) - 0.5, taps clamped to the CROP.  fp32 throughout; no handle, no allocation.
 *
 * mra_video_crop_table: host only, no GPU.  One axis of a crop box: idx int16 [n_out][4] (absolute in the source frame, inside
 * [offset, offset + n_src_crop)) and w fp32 [n_out][4], built in float64 and rounded to fp32 once.  MRA_EINVAL with a message for a
 * NULL pointer, a non-positive size, a negative offset, or a crop that ends beyond index 32767 (int16). */
int mra_video_crop_table(int32_t n_src_crop, int32_t offset, int32_t n_out, int16_t* idx, float* w);
#define MRA_VIDEO_QUANT_NONE 0   /* the resized value goes to the normalisation as it is */
#define MRA_VIDEO_QUANT_FLOOR 1  /* the reference's ToUint8 first: floor(min(max(v, 0), 255)) (the clamp is this build's: the bare cast is undefined there) */
/* src uint8 (device), src_bytes: the step's decoded frames, interleaved RGB, [H][W][3] each, concatenated at any byte offsets;
 * frames int64 [n_out][5] (device), per OUTPUT frame
 *   {byte offset of its source frame in src, source height H, source width W, table row, flip (0 / non-zero)};
 * tap_idx int16 / tap_w fp32 [n_tab][2][size][4] (device): per table row the y table then the x table of mra_video_crop_table for one
 * crop box (a clip: its frames share the row; source frames may repeat, as the last-frame padding does; clips of different H x W go in
 * one call); mean[3] / std[3]: HOST arrays; out [n_out][3][size][size], MRA_F32 or MRA_F16 (device), sample-major, what
 * mra_vit_forward reads:
 *   out = ((q(h) / 255) - mean_c) / std_c,  h = the horizontal 4-tap sum over the vertical 4-tap sums, x reversed when flip is set,
 * q = identity or the MRA_VIDEO_QUANT_FLOOR step; two divisions, as the host processor.  With the whole frame as the box and
 * size == H == W the weights are exactly 0 / 1 and the result is the host processor's normalisation of the bytes.
 * One launch of n_out * size / 8 workgroups; the host side does not read the descriptors, allocates nothing and does not synchronise.
 * Inside the kernel every descriptor is clipped: no read outside [0, src_bytes) (such a byte counts as 0), no write outside out.
 * Checked before any launch, MRA_EINVAL with a message: a negative count, an out_dtype or quantize value not listed, size not a
 * positive multiple of 8 or above 768 (what one workgroup's LDS holds: 8 output rows x 3 channels x size columns of fp32, the 12
 * source rows under them and the x table), NULL mean / std, std <= 0, non-finite mean / std; and, with n_out > 0, a NULL pointer, n_tab < 1, frames /
 * tap_idx not 8-byte or tap_w / out not 16-byte aligned.  n_out == 0 is a no-op. */
int mra_video_frames_forward(const void* src, int64_t src_bytes, const int64_t* frames, int32_t n_out, const int16_t* tap_idx,
                             const float* tap_w, int32_t n_tab, int32_t size, const float* mean, const float* std, int32_t quantize,
                             void* out, int32_t out_dtype, void* stream);
/* algorithmic bytes of such a call with every source frame read once: n_out * (3 src_h src_w + 3 size^2 sizeof(out element)) */
double mra_video_frames_bytes(int64_t n_out, int32_t src_h, int32_t src_w, int32_t size, int32_t out_dtype);
/* mra_video_frames_forward with the kernel's form chosen: 0 = as the product entry (source rows and vertical sums staged in LDS where the
 * crop does not downscale, otherwise the gather), 1 = every workgroup gathers its 16 taps per output from global memory.  Same bits. */
int mra_debug_video_frames_forward(const void* src, int64_t src_bytes, const int64_t* frames, int32_t n_out, const int16_t* tap_idx,
                                   const float* tap_w, int32_t n_tab, int32_t size, const float* mean, const float* std, int32_t quantize,
                                   void* out, int32_t out_dtype, int32_t form, void* stream);

/* ---- diagnostics (no reference counterpart) ---------------------------------------------------------------
 * Number of GEMM launches of one main loop ("family") with one epilogue since the library was loaded; read-only, the only
 * process-wide state of the library.  `family` is a GemmFamily and `epilogue` a GemmEpi of csrc/kernels.h (the numbers mraudio_amd/_lib.py
 * repeats as GF_* and EPI_*): families 0 .. 13 -- the two-buffer, loader-wave, eight-phase, 128-deep and ring main loops, one per tile --
 * and epilogues 0 .. 13.
 * Returns -1 for an unknown family / epilogue.  Used by the parity tests to state which kernel produced the numbers checked. */
int64_t mra_debug_gemm_launches(int32_t family, int32_t epilogue);

/* One stage of an encoder on its own, through the SAME launch code as the forward (kernel selection, LDS and bucket table included), for the
 * per-kernel tests against float64 (tests/test_gpu_encoder_cores.py).  Buffers are device pointers in the kernels' own layouts; arguments are
 * checked as the forwards check theirs: a null handle or pointer, a negative n, a layer or token count out of range -> MRA_EINVAL before any
 * launch; n == 0 is a no-op; no allocation beyond the forward's (the bucket table of a new token count, cached per handle).
 *
 * mra_debug_vit_attention: the attention core of one ViT block over n frames of S = (img / patch)^2 + 1 tokens.  No parameter needs to be loaded.
 *   qkv [n * S][3][heads][96]  operand dtype: q, k, v of a token, each head padded from hd = dim / heads to 96 columns; columns hd .. 95 of
 *                              every head MUST be zero (the padded QKV weight makes them so in the forward)
 *   ctx [n * S][heads * hd]    operand dtype: softmax(q k^T / sqrt(hd)) v per (frame, head), heads side by side, unpadded
 * Follows the handle's "attn_persist" option at S = 257.
 *
 * mra_debug_beats_attention: the attention core of layer `layer` over n chunks of `tokens` (1 .. 512) tokens, with the gated relative-position
 * bias.  Needs encoder.layers.0.self_attn.relative_attention_bias.weight and the layer's self_attn.grep_linear.{weight,bias} and
 * self_attn.grep_a loaded (MRA_ESTATE otherwise).
 *   qkv      [n * tokens][3 * dim]  f16: q | k | v rows as the QKV GEMM writes them (q unscaled), head h at columns 64 h .. 64 h + 63 of each third
 *   gate_src [n * tokens][dim]      f16: the layer input, read in MRA_BEATS_GATE_INPUT mode only; ignored (may be NULL) in MRA_BEATS_GATE_Q
 *                                   mode, where the gate reads the q third of qkv
 *   ctx      [n * tokens][dim]      f16: softmax(q k^T / 8 + G[i] E[bucket(j - i)][h]) v, heads side by side
 *
 * mra_debug_beats_posconv: x += GELU(grouped positional convolution of x) over n chunks of `tokens` tokens.  Needs encoder.pos_conv.0.weight
 * (the effective weight) and encoder.pos_conv.0.bias loaded (MRA_ESTATE otherwise).
 *   x [n * tokens][dim]  fp32, updated in place; the convolution reads x rounded to f16
 *
 * mra_debug_shared_kv_attention: the cross core of mra_qformer_forward_multi on its own, through the forward's launch code (grid split of long
 * KV included).  No handle, no parameters.
 *   q   [enc_items * prompts][32][heads * 64]  operand dtype (MRA_F16 / MRA_BF16): row i * prompts + p = encoder item i, prompt slot p
 *   k,v [enc_items][heads][kv][64]             operand dtype: one layer of the K/V cache's layout
 *   ctx [enc_items * prompts][32][heads * 64]  operand dtype: softmax(q k^T / 8) v of chain item n over the K/V of item n / prompts
 *   core 0: attn_kernel with kv_share, 1: the shared-stream core.  workspace (16-byte aligned) holds the grid-split partials:
 *   mra_debug_shared_kv_workspace_bytes (0 where the core does not split).  enc_items == 0 is a no-op. */
int mra_debug_vit_attention(mra_vit* h, const void* qkv, int32_t n, void* ctx, void* stream);
size_t mra_debug_shared_kv_workspace_bytes(int32_t enc_items, int32_t prompts, int32_t heads, int32_t kv, int32_t core);
int mra_debug_shared_kv_attention(const void* q, const void* k, const void* v, int32_t dtype, int32_t enc_items, int32_t prompts,
                                  int32_t heads, int32_t kv, int32_t core, void* ctx, void* workspace, size_t workspace_bytes, void* stream);
int mra_debug_beats_attention(mra_beats* h, int32_t layer, const void* qkv, const void* gate_src, int32_t n, int32_t tokens, void* ctx,
                              void* stream);
int mra_debug_beats_posconv(mra_beats* h, float* x, int32_t n, int32_t tokens, void* stream);
/* mra_debug_attention_bwd: the attention backward core on its own in the cross-attention layout of mra_qformer_backward(_multi), through
 * launch_attn_bwd.  No handle, no parameters, no mask.  `share` chain items stand behind one K/V item (1: every item its own).
 *   q, o, d_o, dq [kv_items * share][q_rows][heads * 64]  operand dtype (MRA_F16 / MRA_BF16): row block i * share + p = K/V item i, slot p
 *   k, v, dk, dv  [kv_items][heads][kv][64]               operand dtype; dk / dv of item i are summed over its `share` slots
 *   lse           [kv_items * share][heads][q_rows]       fp32 log2-sum-exp2 of the scaled scores (AttnArgs::lse)
 * MRA_EINVAL with a message for a NULL pointer, a non-positive size, a dtype that is not f16 / bf16, and a share (or q_rows) whose fp32
 * dQ / lse / delta areas pass 160 KB of LDS: share * ceil(q_rows / 32) <= 14. */
int mra_debug_attention_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse, int32_t dtype,
                            int32_t kv_items, int32_t share, int32_t heads, int32_t q_rows, int32_t kv, void* dq, void* dk, void* dv, void* stream);

/* The Q-Former forward's own kernels, one launch each, through the launch functions the forward calls (tests/test_gpu_qformer_kernels.py).  No
 * handle, no parameters, no allocation; buffers are device pointers in the kernels' own layouts.  Arguments are checked before any launch: a
 * null pointer, a bad size or a misaligned buffer -> MRA_EINVAL; zero rows / items is a no-op that returns 0.  `dtype` is the operand dtype
 * (MRA_F16 / MRA_BF16).  A row view is a HOST triple int64 {item_stride, rows per item, row stride} in elements (csrc/kernels.h RowView:
 * logical row m lives at (m / rpi) * item_stride + (m % rpi) * stride).
 *
 * mra_debug_self_attention: the masked self-attention core of a layer, built by the forward's own argument builder for hidden = heads * 64.
 *   qkv  [items][S][3 * heads * 64]  q | k | v rows as the QKV GEMM writes them; K and V are read in place
 *   mask [items][S] int64 (1 = attend; additive (1 - m) * -10000) or NULL = all ones (the unmasked kernels)
 *   ctx  [items][S][heads * 64]      lse [items][heads][S] fp32 log2-sum-exp2 of the scaled, masked scores, or NULL
 * mra_debug_self_attention_bwd: the attention backward core (launch_attn_bwd) in the self-attention layout of mra_qformer_backward(_multi),
 *   built by the training step's own argument builder for hidden = heads * 64: Q, K and V are read in place from the packed rows.
 *   qkv, mask     as mra_debug_self_attention takes them (mask NULL = no mask term: all ones)
 *   ctx, d_ctx    [items][S][heads * 64]  the forward's context rows and their upstream gradient, operand dtype
 *   lse           [items][heads][S]       fp32, log2 units, mask included (what mra_debug_self_attention writes)
 *   dqkv          [items][S][3 * heads * 64]  dq | dk | dv, the layout of qkv; every column of every row is written
 *   MRA_EINVAL with a message, nothing written: a NULL pointer other than mask, items / S / heads < 1, a dtype that is not f16 / bf16, a
 *   misaligned buffer, S > 448 (the fp32 dQ / lse / delta areas of ceil(S / 32) > 14 query blocks pass 160 KB of LDS).
 * mra_debug_ln_rows: launch_ln_rows4.  params: HOST array of 8 device pointers gain1, bias1, .. gain4, bias4 (sets 2 - 4 may be NULL pairs);
 *   rows >= lane_rows take sets (3, 4) for (1, 2); with a second set of the pair, rows with row % period >= split take it.  Either output
 *   may be NULL (not both).
 * mra_debug_embed_ln: launch_embed_ln.  query [1 or items][Q][H] with query_item_stride 0 or Q * H; ids outside [0, vocab) are clamped;
 *   h32 / h16 [items][Q + L][H] both required, pre32 (the rows before the LayerNorm) optional.
 * mra_debug_modality_ln: launch_modality_ln with explicit width and parameters (mra_modality_ln takes them from a handle, whose enc_width
 *   is a multiple of 64; the kernel takes any multiple of 8 up to 4096).
 * mra_debug_softmax_rows / _fold_rowfactor / _softmax_rescale / _transpose_pad: the folded cross-attention's helpers (csrc/kernels.h states
 *   the layouts); hist [256] int32 or NULL selects the probe variants.
 * mra_debug_split: kind 0 launch_split_rows (src_view, chunk, parts 2 / 3), 1 launch_split_weight (rows x C), 2 launch_split_key_weight
 *   (rows = heads, C = enc_width); src_view, chunk and parts are read by kind 0 only. */
int mra_debug_self_attention(const void* qkv, const int64_t* mask, int32_t dtype, int32_t items, int32_t S, int32_t heads, void* ctx, float* lse,
                             void* stream);
int mra_debug_self_attention_bwd(const void* qkv, const int64_t* mask, const void* ctx, const void* d_ctx, const float* lse, int32_t dtype,
                                 int32_t items, int32_t S, int32_t heads, void* dqkv, void* stream);
int mra_debug_ln_rows(const float* x, const int64_t* x_view, int32_t rows, int32_t H, const float* const* params, int32_t lane_rows, int32_t period,
                      int32_t split, float eps, float* y32, const int64_t* y32_view, void* y16, const int64_t* y16_view, int32_t dtype, void* stream);
int mra_debug_embed_ln(const int64_t* ids, int32_t items, int32_t L, int32_t Q, int32_t H, int32_t vocab, const float* query, int64_t query_item_stride,
                       const float* word, const float* pos, const float* gain, const float* bias, float eps, float* h32, void* h16, float* pre32,
                       int32_t dtype, void* stream);
int mra_debug_modality_ln(const void* x, int32_t x_dtype, const int64_t* item_index, int32_t items, int32_t tokens, int32_t E, const float* gain,
                          const float* bias, float eps, void* out, int32_t dtype, void* stream);
int mra_debug_softmax_rows(const float* S, int64_t ld_s, void* P, int64_t ld_p, int32_t rows, int32_t kv, int32_t kvp, float scale, int32_t dtype,
                           void* stream);
/* mra_debug_fold_query: steps 5 + 6a of a folded cross-attention layer in ONE launch (mra_qformer_set_option "cross_fuse" bit 1; the default
 * folded plan takes it): per head Q_h = x W_q,h^T + b_q,h over the `rows` compact query rows behind x_view (item stride, rows per item, row
 * stride; K = H), rounded to the operand dtype, then q_prime[item][head * Q + q][0 .. E) = Q_h W_k,h with w_k the per-head [E][64] blocks
 * (heads of 64 dims; H, E multiples of 64; rows a multiple of Q).  Bit-identical to the two GEMM launches it replaces.  b_q may be NULL.  Each
 * *_bytes is the size of its buffer: a view or a size that leaves it is refused, like every null or misaligned (16 bytes) buffer, before the
 * launch.  mra_debug_fold_query_launches: such launches since the library was loaded (the forward's included). */
int mra_debug_fold_query(const void* x, const int64_t* x_view, size_t x_bytes, const void* w_q, size_t w_q_bytes, const float* b_q, size_t b_q_bytes,
                         const void* w_k, size_t w_k_bytes, void* q_prime, size_t q_prime_bytes, int32_t rows, int32_t H, int32_t E, int32_t Q,
                         int32_t heads, int32_t dtype, void* stream);
int64_t mra_debug_fold_query_launches(void);
/* mra_debug_qkv_attention: steps 1 + 2 of a layer in ONE launch (mra_qformer_set_option "self_fuse"), hidden H = heads * 64:
 *   rows [items][S][H], wqkv [3 H][H], bqkv [3 H] fp32 or NULL, mask [items][S] int64 or NULL (as mra_debug_self_attention), ctx [items][S][H].
 * ctx is what mra_debug_gemm on a ring tile followed by mra_debug_self_attention gives, bit for bit.  S > 64 is outside the launch's plan:
 * MRA_EINVAL, like every null or misaligned (16 bytes) buffer, before any launch; zero items is a no-op.
 * mra_debug_qkv_attention_launches: such launches since the library was loaded (the forward's included).  mra_debug_attention_launches:
 * launches of the one-wave-per-unit attention core, masked != 0 the masked form (the self-attention of a layer), 0 the unmasked one.
 * mra_debug_self_fuse_plan: 1 when a forward of `lanes` lanes (2 = the pair forward) of `items` items with S rows each, `hidden` and `heads`
 * takes the fused launch under the values `option` of "self_fuse" and `chain_ring` of "chain_ring", 0 when it keeps the two launches;
 * want_full != 0: the forward returns the full sequence (out_full), which keeps them too (no GPU needed). */
int mra_debug_qkv_attention(const void* rows, const void* wqkv, const float* bqkv, const int64_t* mask, int32_t dtype, int32_t items, int32_t S,
                            int32_t heads, void* ctx, void* stream);
int64_t mra_debug_qkv_attention_launches(void);
int64_t mra_debug_attention_launches(int32_t masked);
int32_t mra_debug_self_fuse_plan(int32_t option, int32_t chain_ring, int32_t lanes, int32_t items, int32_t S, int32_t hidden, int32_t heads,
                                 int32_t dtype, int32_t want_full);
/* launches of the row-factor kernel (mra_debug_fold_rowfactor and the forwards' step 6c, plain and probe) since the library was loaded */
int64_t mra_debug_fold_rowfactor_launches(void);
int mra_debug_fold_rowfactor(const float* stat_m, const float* stat_l, float* factors, int32_t rows, int32_t R, int32_t ntiles, void* P, int64_t ld_p,
                             int32_t tile_cols, int32_t kvp, int32_t* hist, void* stream);
int mra_debug_softmax_rescale(void* P, int64_t ld_p, const float* stat_m, const float* stat_l, int32_t rows, int32_t ntiles, int32_t tile_cols,
                              int32_t kvp, int32_t dtype, int32_t* hist, void* stream);
int mra_debug_transpose_pad(const void* src, void* dst, int32_t R, int32_t C, int32_t ld_d, int64_t src_bs, int64_t dst_bs, int32_t batch, int32_t dtype,
                            void* stream);
int mra_debug_split(int32_t kind, const float* src, const int64_t* src_view, int32_t rows, int32_t C, int32_t chunk, int32_t parts, void* dst,
                    int32_t dtype, void* stream);

/* The Q-Former training step's own kernels, one launch each, through the launch functions mra_qformer_forward_train / mra_qformer_backward
 * call (tests/test_gpu_train_kernels.py).  Same rules as the block above: no handle, no allocation, device pointers in the kernels' own
 * layouts, every argument checked before any launch (MRA_EINVAL with a message).  Per-job arguments are HOST arrays with one entry per job;
 * row views are HOST triples, three int64 per view, one after the other.  The entries cannot know the size of a buffer: the caller owns
 * every element the views, strides and sizes address.
 *
 * mra_debug_gemm_tn_group: launch_gemm_tn_group over njobs = 1 .. 4 weight gradients (one job reaches launch_gemm_tn, as in the training step):
 *   dW[n][k] (+)= sum_m dY[m][n] X[m][k], db[n] += sum_m dY[m][n].  Job i: dY[i] / X[i] operand dtype, given as 64-column blocks -- block b of
 *   dY starts at dY + b * y_block_stride[i], its row m at the row view y_views[3 i ..] (csrc/kernels.h GemmTnArgs); dW[i] fp32 [N][ldw];
 *   db NULL, or an array whose entries may be NULL; accumulate[i] != 0: dW += (db always accumulates).
 *   Refused: njobs outside 1 .. 4; a NULL dY / X / dW; dY or X not 16-byte aligned; a view with rows per item <= 0 or a row / item stride that
 *   is not a multiple of 8; a block stride that is not a multiple of 8; M <= 0; N or K not a positive multiple of 64; ldw < K; and a group
 *   whose contraction the launcher splits while one of its jobs does not accumulate.
 * mra_debug_ln_bwd: launch_ln_bwd2 over job a and an optional job b (ptrs_b NULL: none; either job may have 0 rows).  ptrs_*: HOST array of 8
 *   device pointers dy, x, gamma, dx, add, dx16, dgamma, dbeta (add, dx16 and the dgamma / dbeta pair may be NULL); views_*: 5 views dy, x, dx,
 *   add, dx16 (those of NULL buffers are not read).  dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ add), g = dy gamma; dx16 = dx rounded
 *   once; dgamma += sum_rows dy xhat, dbeta += sum_rows dy.
 *   Refused: H outside {256, 512, 768, 1024}; negative rows; a NULL dy / x / gamma / dx of a job with rows; a view whose strides are not
 *   multiples of 4 (8 for dx16) or whose row stride is below H; a buffer that is not 16-byte aligned; dgamma without dbeta (or the reverse);
 *   two jobs of which only one takes dgamma.
 * mra_debug_embed_bwd: launch_embed_bwd.  demb [items][Q + L][H] fp32; dquery [Q][H] += sum over items, dpos [L][H] likewise, dword
 *   [vocab][H] += the rows of the ids (clamped to [0, vocab) as the forward clamps them); each output may be NULL.  items == 0 is a no-op.
 *   Refused: H <= 0 or H % 4; Q < 0, L < 0 or Q + L == 0; vocab < 1; negative items; NULL demb; NULL ids with L > 0 and dword given.
 * mra_debug_transpose16_batch: launch_transpose16_batch over njobs = 1 .. 64 matrices, dst[i] [C][R] = src[i] [R][C]^T (operand dtype).  The
 *   job table is built as the training step builds it and copied (synchronously) into `scratch`, device memory of at least
 *   mra_debug_transpose16_batch_scratch_bytes(njobs) bytes (0 for an njobs out of range), 8-byte aligned.
 *   Refused: njobs out of range, R or C below 1, a NULL matrix, a scratch buffer that is NULL, too small or misaligned.
 * mra_debug_gemm_gelu: one or two problems C = A W^T through launch_gemm, as Ctx::gemm2 (csrc/mra_train.hip) issues the feed-forward
 *   up-projection and its data gradient.  backward == 0: EPI_GELU_BOTH, aux = T(acc + bias), C = T(gelu(aux)); backward != 0: EPI_GELU_BWD,
 *   C = T(acc gelu'(aux)), aux read.  W[i] [N][K] dense; A by a_views, C and aux by c_views; bias NULL or an array with NULL entries.
 *   tile_cfg: GT_AUTO (0), GT_64 (1), GT_128 (2), GT_256 (3) of csrc/kernels.h.
 *   Refused: what gemm_plan refuses (M, N or K <= 0, K % 64, N no multiple of the tile, C strides no multiples of 4), a NULL A / W / C / aux,
 *   A strides that are not multiples of 8, a row stride below the row length, a misaligned buffer (A, W, bias 16 bytes; C, aux 8). */
int mra_debug_gemm_tn_group(int32_t njobs, const void* const* dY, const int64_t* y_views, const int64_t* y_block_stride, const void* const* X,
                            const int64_t* x_views, const int64_t* x_block_stride, float* const* dW, float* const* db, const int32_t* M,
                            const int32_t* N, const int32_t* K, const int32_t* ldw, const int32_t* accumulate, int32_t dtype, void* stream);
int mra_debug_ln_bwd(const void* const* ptrs_a, const int64_t* views_a, int32_t rows_a, float eps_a, const void* const* ptrs_b, const int64_t* views_b,
                     int32_t rows_b, float eps_b, int32_t H, int32_t dtype, void* stream);
int mra_debug_embed_bwd(const float* demb, const int64_t* ids, int32_t items, int32_t L, int32_t Q, int32_t H, int32_t vocab, float* dquery, float* dpos,
                        float* dword, void* stream);
size_t mra_debug_transpose16_batch_scratch_bytes(int32_t njobs);
int mra_debug_transpose16_batch(const void* const* src, void* const* dst, const int32_t* R, const int32_t* C, int32_t njobs, int32_t dtype, void* scratch,
                                size_t scratch_bytes, void* stream);
int mra_debug_gemm_gelu(int32_t nprob, const void* const* A, const int64_t* a_views, const void* const* W, const float* const* bias, void* const* C,
                        const int64_t* c_views, void* const* aux, const int32_t* M, const int32_t* N, const int32_t* K, int32_t backward, int32_t tile_cfg,
                        int32_t dtype, void* stream);

/* The forward GEMMs, one launch each, through launch_gemm (tests/test_gpu_gemm_forward.py): the launch forms of mra_qformer_forward*,
 * mra_kv_project and mra_llm_proj.  No handle, no allocation.  A launch is 1 .. 4 problem descriptors; the descriptor mirrors the GemmProb
 * fields of csrc/kernels.h that those forwards set (see there for their meaning) and ADDS the byte size of every buffer handed over, so
 * the entry can check the whole read and write footprint on the host before anything is launched.
 *   struct_bytes   sizeof(mra_gemm_desc) as the caller sees it; a mismatch is refused, not misread
 *   *_view         row views, HOST triples {item_stride, rows per item, row stride} in elements
 *   *_bytes        bytes addressable from the pointer of the same name (0 with a NULL pointer)
 * mra_debug_gemm: epilogue one of EPI_OP, EPI_GELU_OP, EPI_RES_F32, EPI_F32, EPI_KV, EPI_SOFTPART, EPI_RES_LN (0 .. 5, 9) or one of the ViT's
 *   (below); dtype MRA_F16 /
 *   MRA_BF16.  gemm_plan runs first (it picks the tile every footprint below is computed with); then refused with MRA_EINVAL and a message:
 *   a NULL A / W / C; A, W, C, R, bias, the LayerNorm buffers or pscale not 16-byte aligned (stat_m, stat_l, ln_counter: 4); an A view whose
 *   strides are not multiples of 8 or a batch stride the vector accesses cannot take (a_bs, w_bs: 8 elements; c_bs_bytes: 16 bytes;
 *   bias_bs: 4); a row stride below the row length (A: K; C, R and the LayerNorm outputs: the columns
 *   written, i.e. ceil(N / tile) * tile with n_ragged and for EPI_SOFTPART); w_ld < N; a negative batch or stride; and ANY problem whose
 *   footprint leaves the given sizes --
 *     A        rows of the view x K elements, + (batch - 1) a_bs
 *     W        [N][K] ([N][K / 2] with w_kwrap; (k_rows - 1) w_ld + N with w_ld), + (batch - 1) w_bs
 *     bias     N floats, + (batch - 1) bias_bs
 *     C, R     rows of the view x columns written, + (batch - 1) c_bs_bytes (R is not batched); EPI_KV: (N / (kv_heads * 64)) x kv_items x
 *              kv_heads x kv_tokens x 64 elements, with N a multiple of kv_heads * 64 and M <= kv_items * kv_tokens
 *     stat_*   batch x M x ntiles floats          pscale   batch x ps_ntiles x 512 floats (M <= 384)
 *     col_scale  N floats, + (batch - 1) cs_bs (EPI_SOFTPART on the 176 x 384 tile only; cs_bs >= N with a batch)
 *     ln_*     N floats of gain and bias, the output rows of the views, ceil(M / 64) counters; the counter ranges of two EPI_RES_LN problems
 *              of one launch must not overlap
 *   What the entry cannot see is device DATA: with pscale the caller keeps A zero from column ps_ntiles * 176 on, and the counters zero.
 *   The ViT encoder's launches (csrc/vit.hip; tests/test_gpu_gemm_vit.py): epilogues EPI_RES_OP, EPI_RES_F32_STAT, EPI_LNF_OP, EPI_LNF_GELU_OP,
 *   EPI_RES_OP_STAT (8, 10 .. 13) and tile_cfg GT_P8_MIXED (N = 256 k + 128 >= 384, K % 128 == 0; GT_P8_TAIL has no shipped call site and stays
 *   refused).  One plain problem each: nprob > 1, a batch or n_ragged is refused.  Under them the LayerNorm fields mean other things --
 *     aux      (8, 13) required, 16-byte aligned, the C footprint in the operand dtype; aux == C (in place) or no overlap with C at all
 *     ln_y32   (11, 12) READ: M x 2 floats of (mean, rstd) per row; (10) WRITTEN: M x (N / 128) x 2 floats of (mean, sum of squared
 *              deviations) per row and 128-column group; (13) the same per 64-column block, M x (N / 64) x 2.  8-byte aligned; ln_y32_view
 *              is ignored
 *     ln_gain  (11, 12) N floats: the column sums of the folded weight; ln_bias is not read
 *     ln_y16   (10) the rows once more in the operand dtype: rows of ln_y16_view (strides multiples of 8) x N elements, 16-byte aligned
 *     bias     (10, 13) required, N floats;  R (10) as for EPI_RES_F32
 *   and whatever epilogue_rules / tile_rules of csrc/gemm.hip refuse for them is MRA_EINVAL here, never a launch.
 * mra_debug_gemm_plan: host only, no GPU needed and no pointer followed: the same checks over the same descriptors -- every refusal above --
 *   and gemm_plan for a device of `cus` compute units, without the launch.  out[0 .. 6] = tile (GemmTile), family (GemmFamily), threads, LDS
 *   bytes, grid, persistent flag, total tiles. */
typedef struct mra_gemm_desc {
  uint64_t struct_bytes;
  const void* A; const void* W; const float* bias; void* C; const float* R;
  int64_t a_view[3], c_view[3], r_view[3];
  int32_t M, N, K;
  int32_t kv_tokens, kv_items, kv_heads;
  int32_t batch, bias_bs;
  int64_t a_bs, w_bs, c_bs_bytes;
  int32_t n_ragged, w_ld, k_rows, w_kwrap;
  const float* ln_gain; const float* ln_bias; float* ln_y32; void* ln_y16; uint32_t* ln_counter;
  int64_t ln_y32_view[3], ln_y16_view[3];
  float ln_eps, alpha;
  float* stat_m; float* stat_l; const float* pscale;
  int32_t ps_ntiles, tile_cfg, persist, reserved;
  uint64_t a_bytes, w_bytes, bias_bytes, c_bytes, r_bytes, ln_gain_bytes, ln_bias_bytes, ln_y32_bytes, ln_y16_bytes, ln_counter_bytes, stat_m_bytes,
      stat_l_bytes, pscale_bytes;
  /* EPI_SOFTPART on the 176 x 384 tile over RAW weight-side rows (appended; all zero = off): column n of batch entry b carries the factor
   * col_scale[b * cs_bs + n] -- read, or with col_stats = 1 computed in the launch from the rows themselves (1 / sqrt(biased variance over K
   * + cs_eps)) and written there for n < N.  C = T(exp2(alpha r acc - stat_m) r), stat_m over r acc, stat_l the fp32 sum of the exponentials. */
  float* col_scale; int64_t cs_bs; int32_t col_stats; float cs_eps;
  uint64_t col_scale_bytes;
  /* EPI_RES_OP / EPI_RES_OP_STAT (appended; NULL otherwise): the residual in the operand dtype, addressed with c_view.  aux == C updates the
   * stream in place; any other overlap with C is refused. */
  void* aux; uint64_t aux_bytes;
  /* tile_cfg GT_64 only (appended; 0 = off): k128 = 1 takes the 64 x 64 tile with 128-deep K steps (family 10) whenever K % 128 == 0, not only
   * from K = 2048 on -- the folded context GEMM under mra_qformer_set_option "cross_fuse" bit 4. */
  /* EPI_OP over K-major weights on the 176 x 384 tile (appended; 0 = off): ps_stats = 1 feeds the launch the tile statistics of the scores
   * launch -- stat_m / stat_l, batch x M x ps_ntiles floats, M <= 384 -- instead of pscale (which must be NULL): it computes the row factors
   * exp2(m_tile - m_row) / L_row itself, bit for bit those of mra_debug_fold_rowfactor, and A need not be zero from column ps_ntiles * 176
   * on (mra_qformer_set_option "cross_fuse" bit 2). */
  int32_t k128, ps_stats;
} mra_gemm_desc;
int mra_debug_gemm(const mra_gemm_desc* probs, int32_t nprob, int32_t epilogue, int32_t dtype, void* stream);
int mra_debug_gemm_plan(const mra_gemm_desc* probs, int32_t nprob, int32_t epilogue, int32_t dtype, int32_t cus, int32_t* out);

/* The companions of the ViT's folded LayerNorm (csrc/vit.hip), one launch each through the launch forms of mra_vit_forward
 * (tests/test_gpu_gemm_vit.py).  No handle, no allocation; device pointers, every buffer with its size in bytes; `dtype` is the operand dtype
 * (MRA_F16 / MRA_BF16).  Checked on the host before the launch, MRA_EINVAL with a message: a NULL or misaligned buffer, a size out of range,
 * a footprint that leaves the given bytes.  Zero rows is a no-op.
 * mra_debug_vit_fold_weight: W [N][K] operand dtype, gain / beta [K], bias [N] or NULL -> Wf [N][K] = T(w gain), cs [N] = the row sums of
 *   the ROUNDED Wf, bf [N] = bias + sum_k beta w.  Wf may be W itself; any other overlap is refused.
 * mra_debug_vit_group_stats: groups [M][G] float2 (mean, sum of squared deviations) of group_cols columns each -> stats [M] float2
 *   (mean, 1 / sqrt(variance + eps)) of the whole row.  G and group_cols 1 .. 4096; groups and stats 8-byte aligned.
 * mra_debug_vit_row_stats: x [M][D] -> stats [M] float2 (mean, rstd).  x_dtype MRA_F32: x fp32 (8-byte aligned) and x16 [M][D] receives the
 *   rows in the operand dtype; x_dtype == dtype: x in the operand dtype, x16 must be NULL.  D a multiple of 128, at most 2048. */
int mra_debug_vit_fold_weight(const void* W, size_t w_bytes, const float* gain, size_t gain_bytes, const float* beta, size_t beta_bytes, const float* bias,
                              size_t bias_bytes, void* Wf, size_t wf_bytes, float* cs, size_t cs_bytes, float* bf, size_t bf_bytes, int32_t N, int32_t K,
                              int32_t dtype, void* stream);
int mra_debug_vit_group_stats(const float* groups, size_t groups_bytes, int64_t M, int32_t G, int32_t group_cols, float eps, float* stats,
                              size_t stats_bytes, void* stream);
int mra_debug_vit_row_stats(const void* x, size_t x_bytes, int32_t x_dtype, int64_t M, int32_t D, float eps, float* stats, size_t stats_bytes, void* x16,
                            size_t x16_bytes, int32_t dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MRA_H_ */
