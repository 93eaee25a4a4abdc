// Backward of the LLM projection (row A5, models/xinstructblip.py:303; not in the reference, which never trains through it on this path):
//     y[R][Lh] = op(z)[R][H] W[Lh][H]^T + b,   op = rounding to the operand dtype,   dY = op(upstream gradient)
//   d_z[R][H]  = dY W            written.  The contraction runs over Lh and W as stored is k-major, the wrong way round for an MFMA operand:
//                                kvgrad_gemm_kernel's row-major mode (enc_grad.hip: launch_rowgrad_gemm) reads it through the LDS transpose
//                                read.  No transposed copy of llm_proj.weight exists: the weight is trained, a copy would go stale every step.
//   d_W[Lh][H] += dY^T op(z),  d_b[Lh] += colsum(dY)      one launch_gemm_tn (gemm_tn.hip) with its db output.
// The rounding of z is passed straight through, like every 16-bit tensor of the training tape.
#include "mra_handle.h"

using namespace mra;
using namespace mra_host;

namespace mra {

int launch_llm_proj_bwd(const void* dY, const void* z16, const void* W, int R, int Lh, int H, float* d_z, float* d_W, float* d_b, float* scratch,
                        int op_dtype, hipStream_t stream) {
  if (R <= 0) return 0;
  if (Lh <= 0 || Lh % 64 || H <= 0 || H % 128) return -1;
  if (d_z)
    if (int rc = launch_rowgrad_gemm(dY, W, d_z, R, Lh, H, op_dtype, stream)) return rc;
  if (!d_W && !d_b) return 0;
  GemmTnArgs a{};
  a.dY = dY; a.yv = plain(R, Lh); a.y_block_stride = 64;
  a.X = z16; a.xv = plain(R, H); a.x_block_stride = 64;
  a.M = R; a.N = Lh;
  a.db = d_b;
  if (d_W) {
    a.dW = d_W; a.K = H; a.ldw = H; a.accumulate = 1;
  } else {   // the bias gradient rides on the column-block-0 workgroups: give them one block of X and a throw-away product
    if (!scratch) return -1;
    a.dW = scratch; a.K = 64; a.ldw = 64; a.accumulate = 0;
  }
  return launch_gemm_tn(a, op_dtype, stream);
}

}  // namespace mra

namespace {

struct ProjBwdWs {
  size_t z16, dy16, scratch, bytes;   // offsets; dy16 is used only for an fp32 d_out
};
ProjBwdWs proj_bwd_layout(const mra_cfg& c, int rows, int d_out_dtype) {
  ProjBwdWs w{};
  w.z16 = 0;
  w.dy16 = align_up((size_t)rows * c.hidden * 2);
  w.scratch = w.dy16 + (d_out_dtype == MRA_F32 ? align_up((size_t)rows * c.llm_hidden * 2) : 0);
  w.bytes = w.scratch + align_up((size_t)c.llm_hidden * 64 * 4);
  return w;
}

}  // namespace

extern "C" {

size_t mra_llm_proj_backward_workspace_bytes(mra_qformer* h, int32_t rows, int32_t d_out_dtype) {
  if (!h || rows <= 0 || h->cfg.llm_hidden <= 0) return 0;
  return proj_bwd_layout(h->cfg, rows, d_out_dtype).bytes;
}

int mra_llm_proj_backward(mra_qformer* h, const float* z, int32_t rows, const void* d_out, int32_t d_out_dtype, float* d_z, float* d_weight,
                          float* d_bias, void* workspace, size_t workspace_bytes, void* stream_) {
  if (!h) return fail(MRA_EINVAL, "null handle");
  if (rows < 0) return fail(MRA_EINVAL, "negative rows");
  if (rows == 0) return MRA_OK;
  const mra_cfg& c = h->cfg;
  if (c.llm_hidden <= 0 || !h->params["llm_proj.weight"].loaded || !h->params["llm_proj.bias"].loaded)
    return fail(MRA_ESTATE, "llm_proj not loaded");
  if (c.llm_hidden % 64) return fail(MRA_EINVAL, "llm_hidden must be a multiple of 64");
  if (c.hidden % 128) return fail(MRA_EINVAL, "hidden must be a multiple of 128");
  if (d_out_dtype != MRA_F32 && d_out_dtype != c.op_dtype) return fail(MRA_EINVAL, "d_out_dtype must be f32 or the operand dtype");
  if (!z || !d_out) return fail(MRA_EINVAL, "null z or d_out");
  if ((long long)rows * c.llm_hidden > 0x7fffffffLL) return fail(MRA_EINVAL, "rows * llm_hidden exceeds int32");
  const ProjBwdWs w = proj_bwd_layout(c, rows, d_out_dtype);
  if (!workspace || workspace_bytes < w.bytes) return fail(MRA_ENOMEM, "workspace too small: need " + std::to_string(w.bytes) + " bytes");
  if (reinterpret_cast<uintptr_t>(workspace) % 256) return fail(MRA_EINVAL, "workspace must be 256-byte aligned");
  if (d_out_dtype != MRA_F32 && reinterpret_cast<uintptr_t>(d_out) % 16) return fail(MRA_EINVAL, "d_out must be 16-byte aligned");
  if (!d_z && !d_weight && !d_bias) return MRA_OK;
  hipStream_t stream = as_stream(stream_);
  char* ws = (char*)workspace;
  const void* dy16 = d_out;
  if (d_out_dtype == MRA_F32) {
    if (int rc = launch_convert(d_out, MRA_F32, ws + w.dy16, c.op_dtype, (long long)rows * c.llm_hidden, stream)) return chk(rc, "convert d_out");
    dy16 = ws + w.dy16;
  }
  if (d_weight || d_bias)
    if (int rc = launch_convert(z, MRA_F32, ws + w.z16, c.op_dtype, (long long)rows * c.hidden, stream)) return chk(rc, "convert z");
  return chk(launch_llm_proj_bwd(dy16, ws + w.z16, h->wllm, rows, c.llm_hidden, c.hidden, d_z, d_weight, d_bias, (float*)(ws + w.scratch), h->op(),
                                 stream),
             "llm_proj backward");
}

}  // extern "C"
