// C-ABI plumbing: per-thread error text, launch checks, the program runner, and the thin
// extern "C" entry points that fill an HrOp and call the launcher of the same op kind.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "common.h"

namespace {
thread_local char g_err[512] = "";
}

void hr_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int hr_check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    hr_set_error("%s: HIP launch failed: %s", what, hipGetErrorString(e));
    return HR_E_LAUNCH;
  }
  return HR_OK;
}

extern "C" const char* hrnet_last_error_string(void) { return g_err; }
// 2: HR_CONV_I_ROUTE, HR_WGRAD_I_ATOMIC .. HR_WGRAD_I_LD, HrPackEnt.ld, the head / table op kinds of round 3
extern "C" int hrnet_abi_version(void) { return HR_ABI_VERSION; }

static int run_one(const HrOp& op, hipStream_t s, int k) {
  int e;
  switch (op.kind) {
    case HR_OP_CONV: e = hr_launch_conv(op, s); break;
    case HR_OP_WGRAD: e = hr_launch_wgrad(op, s); break;
    case HR_OP_WGRAD_REDUCE: e = hr_launch_wgrad_reduce(op, s); break;
    case HR_OP_BN_FINALIZE: e = hr_launch_bn_finalize(op, s); break;
    case HR_OP_SUM_TERMS: e = hr_launch_sum_terms(op, s); break;
    case HR_OP_GRAD_TERM: e = hr_launch_grad_term(op, s); break;
    case HR_OP_BN_BWD_REDUCE: e = hr_launch_bn_bwd_reduce(op, s); break;
    case HR_OP_BN_BWD_FINALIZE: e = hr_launch_bn_bwd_finalize(op, s); break;
    case HR_OP_BILINEAR_CAT: e = hr_launch_bilinear_cat(op, s); break;
    case HR_OP_BILINEAR_CAT_BWD: e = hr_launch_bilinear_cat_bwd(op, s); break;
    case HR_OP_IM2COL_STEM: e = hr_launch_im2col_stem(op, s); break;
    case HR_OP_NHWC_TO_NCHW: e = hr_launch_nhwc_to_nchw(op, s); break;
    case HR_OP_NCHW_TO_NHWC: e = hr_launch_nchw_to_nhwc(op, s); break;
    case HR_OP_PACK_WEIGHTS: e = hr_launch_pack_weights(op, s); break;
    case HR_OP_BIAS_GRAD: e = hr_launch_bias_grad(op, s); break;
    case HR_OP_FILL: e = hr_launch_fill(op, s); break;
    case HR_OP_PACK_TABLE: e = hr_launch_pack_table(op, s); break;
    case HR_OP_WGRAD_REDUCE_TABLE: e = hr_launch_wgrad_reduce_table(op, s); break;
    case HR_OP_BWD_FUSED: e = hr_launch_bwd_fused(op, s); break;
    case HR_OP_BWD_PW: e = hr_launch_bwd_pw(op, s); break;
    case HR_OP_CONV_SUM: e = hr_launch_conv_sum(op, s); break;
    case HR_OP_BN_FINALIZE_TABLE: e = hr_launch_bn_finalize_table(op, s); break;
    case HR_OP_EW_TABLE: e = hr_launch_ew_table(op, s); break;
    case HR_OP_HEAD_MIX: e = hr_launch_head_mix(op, s); break;
    case HR_OP_UPSAMPLE_T: e = hr_launch_upsample_t(op, s); break;
    case HR_OP_HEAD_BWD: e = hr_launch_head_bwd(op, s); break;
    case HR_OP_POOL_REDUCE: e = hr_launch_pool_reduce(op, s); break;
    case HR_OP_EVENT_RECORD:
      e = hipEventRecord((hipEvent_t)op.p[HR_EVENT_P_EVENT], s) == hipSuccess ? HR_OK : HR_E_LAUNCH;
      if (e) hr_set_error("event record failed");
      break;
    case HR_OP_STREAM_WAIT:
      e = hipStreamWaitEvent(s, (hipEvent_t)op.p[HR_EVENT_P_EVENT], 0) == hipSuccess ? HR_OK : HR_E_LAUNCH;
      if (e) hr_set_error("stream wait failed");
      break;
    default:
      hr_set_error("program_run: unknown op kind %d at index %d", op.kind, k);
      return HR_E_BADOP;
  }
  if (e != HR_OK) {
    char tmp[400];
    strncpy(tmp, g_err, sizeof(tmp) - 1);
    tmp[sizeof(tmp) - 1] = 0;
    hr_set_error("op %d (kind %d): %s", k, op.kind, tmp);
  }
  return e;
}

extern "C" int hrnet_program_run(const HrOp* ops, int n, hr_stream_t stream) {
  for (int k = 0; k < n; ++k) {
    // single-stream execution is already ordered: lane markers are no-ops
    if (ops[k].kind == HR_OP_EVENT_RECORD || ops[k].kind == HR_OP_STREAM_WAIT) continue;
    const int e = run_one(ops[k], (hipStream_t)stream, k);
    if (e != HR_OK) return e;
  }
  return HR_OK;
}

extern "C" int hrnet_program_run_streams(const HrOp* ops, int n, const hr_stream_t* streams, int nstreams) {
  HR_REQUIRE(streams && nstreams >= 1, "program_run_streams: no streams");
  for (int k = 0; k < n; ++k) {
    const int lane = ops[k].i[HR_LANE_SLOT];
    HR_REQUIRE(lane >= 0 && lane < nstreams, "program_run_streams: op %d lane %d out of range", k, lane);
    const int e = run_one(ops[k], (hipStream_t)streams[lane], k);
    if (e != HR_OK) return e;
  }
  return HR_OK;
}

// The same with a timing event recorded behind every op on its lane: end_ms[k] = when op k was done, in ms since
// the first op's lane reached the start of the call (event ops: when the lane passed them). Synchronises the
// streams before it returns - a measurement entry point (bench.py / scratch timelines), not for the training loop.
extern "C" int hrnet_program_run_streams_timed(const HrOp* ops, int n, const hr_stream_t* streams, int nstreams,
                                               float* end_ms) {
  HR_REQUIRE(streams && nstreams >= 1 && end_ms && n >= 1, "program_run_streams_timed: arguments");
  std::vector<hipEvent_t> ev((size_t)n + 1, nullptr);
  for (auto& e : ev)
    if (hipEventCreate(&e) != hipSuccess) { hr_set_error("program_run_streams_timed: event create"); return HR_E_LAUNCH; }
  int rc = HR_OK;
  const int lane0 = ops[0].i[HR_LANE_SLOT];
  HR_REQUIRE(lane0 >= 0 && lane0 < nstreams, "program_run_streams_timed: lane");
  hipEventRecord(ev[n], (hipStream_t)streams[lane0]);
  int done = 0;
  for (int k = 0; k < n && rc == HR_OK; ++k, ++done) {
    const int lane = ops[k].i[HR_LANE_SLOT];
    if (lane < 0 || lane >= nstreams) { hr_set_error("program_run_streams_timed: op %d lane %d", k, lane); rc = HR_E_BADARG; break; }
    rc = run_one(ops[k], (hipStream_t)streams[lane], k);
    hipEventRecord(ev[k], (hipStream_t)streams[lane]);
  }
  for (int l = 0; l < nstreams; ++l) hipStreamSynchronize((hipStream_t)streams[l]);
  for (int k = 0; k < done; ++k) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, ev[n], ev[k]);
    end_ms[k] = ms;
  }
  for (auto& e : ev) hipEventDestroy(e);
  return rc;
}

extern "C" void* hrnet_event_create(void) {
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
    hr_set_error("hipEventCreate failed");
    return nullptr;
  }
  return (void*)ev;
}

extern "C" int hrnet_event_destroy(void* event) {
  return hipEventDestroy((hipEvent_t)event) == hipSuccess ? HR_OK : HR_E_LAUNCH;
}

#define OP_BEGIN(KIND) \
  HrOp op;             \
  memset(&op, 0, sizeof(op)); \
  op.kind = KIND

extern "C" int hrnet_wgrad_reduce(const float* slabs, float* grad_oihw, int nsplit, int Cout, int Cin,
                                  int ks, int Cout_real, int Cin_real, int kflat, int accumulate,
                                  hr_stream_t stream) {
  OP_BEGIN(HR_OP_WGRAD_REDUCE);
  op.i[HR_WGRAD_REDUCE_I_NSPLIT] = nsplit; op.i[HR_WGRAD_REDUCE_I_COUT_PAD] = Cout;
  op.i[HR_WGRAD_REDUCE_I_CIN_PAD] = Cin; op.i[HR_WGRAD_REDUCE_I_KS] = ks; op.i[HR_WGRAD_REDUCE_I_COUT] = Cout_real;
  op.i[HR_WGRAD_REDUCE_I_CIN] = Cin_real; op.i[HR_WGRAD_REDUCE_I_KFLAT] = kflat;
  op.i[HR_WGRAD_REDUCE_I_ACCUMULATE] = accumulate;
  op.p[HR_WGRAD_REDUCE_P_SLABS] = (void*)slabs; op.p[HR_WGRAD_REDUCE_P_GRAD] = grad_oihw;
  return hr_launch_wgrad_reduce(op, (hipStream_t)stream);
}

extern "C" int hrnet_pack_weights(int dtype, const float* w_oihw, void* packed, int Cout, int Cin, int ks,
                                  int Cout_pad, int Cin_pad, int mode, hr_stream_t stream) {
  OP_BEGIN(HR_OP_PACK_WEIGHTS);
  op.i[HR_PACK_I_DTYPE] = dtype; op.i[HR_PACK_I_COUT] = Cout; op.i[HR_PACK_I_CIN] = Cin; op.i[HR_PACK_I_KS] = ks;
  op.i[HR_PACK_I_COUT_PAD] = Cout_pad; op.i[HR_PACK_I_CIN_PAD] = Cin_pad; op.i[HR_PACK_I_MODE] = mode;
  op.p[HR_PACK_P_SRC] = (void*)w_oihw; op.p[HR_PACK_P_PACKED] = packed;
  return hr_launch_pack_weights(op, (hipStream_t)stream);
}

extern "C" int hrnet_pack_weights_table(int dtype, const HrPackEnt* table, int n, int total_blocks,
                                        hr_stream_t stream) {
  OP_BEGIN(HR_OP_PACK_TABLE);
  op.i[HR_PACK_TABLE_I_DTYPE] = dtype; op.i[HR_PACK_TABLE_I_N] = n; op.i[HR_PACK_TABLE_I_BLOCKS] = total_blocks;
  op.p[HR_PACK_TABLE_P_TABLE] = (void*)table;
  return hr_launch_pack_table(op, (hipStream_t)stream);
}

extern "C" int hrnet_wgrad_reduce_table(const HrWredEnt* table, int n, int total_blocks, hr_stream_t stream) {
  OP_BEGIN(HR_OP_WGRAD_REDUCE_TABLE);
  op.i[HR_TABLE_I_N] = n; op.i[HR_TABLE_I_BLOCKS] = total_blocks;
  op.p[HR_TABLE_P_TABLE] = (void*)table;
  return hr_launch_wgrad_reduce_table(op, (hipStream_t)stream);
}

extern "C" int hrnet_bn_finalize(const float* stats, int tiles, int C, float count, const float* gamma,
                                 const float* beta, float* running_mean, float* running_var,
                                 int64_t* num_batches_tracked, float momentum, float eps, int training,
                                 float* scale, float* shift, float* save_mean, float* save_invstd,
                                 hr_stream_t stream) {
  OP_BEGIN(HR_OP_BN_FINALIZE);
  op.i[HR_BN_FINALIZE_I_TILES] = tiles; op.i[HR_BN_FINALIZE_I_C] = C; op.i[HR_BN_FINALIZE_I_TRAINING] = training;
  op.f[HR_BN_FINALIZE_F_COUNT] = count; op.f[HR_BN_FINALIZE_F_MOMENTUM] = momentum; op.f[HR_BN_FINALIZE_F_EPS] = eps;
  op.p[HR_BN_FINALIZE_P_STATS] = (void*)stats; op.p[HR_BN_FINALIZE_P_GAMMA] = (void*)gamma;
  op.p[HR_BN_FINALIZE_P_BETA] = (void*)beta; op.p[HR_BN_FINALIZE_P_RUNNING_MEAN] = running_mean;
  op.p[HR_BN_FINALIZE_P_RUNNING_VAR] = running_var; op.p[HR_BN_FINALIZE_P_NUM_BATCHES_TRACKED] = num_batches_tracked;
  op.p[HR_BN_FINALIZE_P_SCALE] = scale; op.p[HR_BN_FINALIZE_P_SHIFT] = shift;
  op.p[HR_BN_FINALIZE_P_SAVE_MEAN] = save_mean; op.p[HR_BN_FINALIZE_P_SAVE_INVSTD] = save_invstd;
  return hr_launch_bn_finalize(op, (hipStream_t)stream);
}

extern "C" int hrnet_sum_terms(int dtype, void* out, int N, int Ho, int Wo, int C, int nterms,
                               const void* const* src, const float* const* scale,
                               const float* const* shift, const int* shifts, const int* relus,
                               int relu_out, hr_stream_t stream) {
  OP_BEGIN(HR_OP_SUM_TERMS);
  HR_REQUIRE(nterms >= 1 && nterms <= 4 && src && shifts && relus, "sum_terms: args");
  op.i[HR_SUM_I_DTYPE] = dtype; op.i[HR_SUM_I_N] = N; op.i[HR_SUM_I_H] = Ho; op.i[HR_SUM_I_W] = Wo;
  op.i[HR_SUM_I_C] = C; op.i[HR_SUM_I_NTERMS] = nterms; op.i[HR_SUM_I_RELU_OUT] = relu_out;
  op.p[HR_SUM_P_OUT] = out;
  for (int t = 0; t < nterms; ++t) {
    op.i[HR_SUM_I_SH0 + t] = shifts[t];
    op.i[HR_SUM_I_RELU0 + t] = relus[t];
    op.p[HR_SUM_P_SRC0 + t] = (void*)src[t];
    op.p[HR_SUM_P_SCALE0 + t] = scale ? (void*)scale[t] : nullptr;
    op.p[HR_SUM_P_SHIFT0 + t] = shift ? (void*)shift[t] : nullptr;
  }
  return hr_launch_sum_terms(op, (hipStream_t)stream);
}

extern "C" int hrnet_sum_terms_bnref(int dtype, void* out, int N, int Ho, int Wo, int C, int nterms,
                                     const void* const* src, const float* const* scale, const float* const* shift,
                                     const int* shifts, const int* relus, int relu_out, int sums_mode,
                                     const float* inv_counts, float eps, hr_stream_t stream) {
  OP_BEGIN(HR_OP_SUM_TERMS);
  HR_REQUIRE(nterms >= 1 && nterms <= 4 && src && shifts && relus && scale && shift && inv_counts, "sum_terms: args");
  op.i[HR_SUM_I_DTYPE] = dtype; op.i[HR_SUM_I_N] = N; op.i[HR_SUM_I_H] = Ho; op.i[HR_SUM_I_W] = Wo;
  op.i[HR_SUM_I_C] = C; op.i[HR_SUM_I_NTERMS] = nterms; op.i[HR_SUM_I_RELU_OUT] = relu_out;
  op.p[HR_SUM_P_OUT] = out;
  for (int t = 0; t < nterms; ++t) {
    op.i[HR_SUM_I_SH0 + t] = shifts[t];
    op.i[HR_SUM_I_RELU0 + t] = relus[t];
    op.p[HR_SUM_P_SRC0 + t] = (void*)src[t];
    op.p[HR_SUM_P_SCALE0 + t] = (void*)scale[t];
    op.p[HR_SUM_P_SHIFT0 + t] = (void*)shift[t];
    op.f[t] = inv_counts[t];
  }
  op.i[HR_SUM_I_SUMS_MODE] = sums_mode;
  memcpy(&op.i[HR_SUM_I_EPS_BITS], &eps, sizeof(float));
  return hr_launch_sum_terms(op, (hipStream_t)stream);
}

extern "C" int hrnet_bn_finalize_table(const HrBnEnt* table, int n, int total_blocks, hr_stream_t stream) {
  OP_BEGIN(HR_OP_BN_FINALIZE_TABLE);
  op.i[HR_TABLE_I_N] = n; op.i[HR_TABLE_I_BLOCKS] = total_blocks;
  op.p[HR_TABLE_P_TABLE] = (void*)table;
  return hr_launch_bn_finalize_table(op, (hipStream_t)stream);
}

extern "C" int hrnet_grad_term(int dtype, void* dst, const void* g, const void* mask_out, const void* y,
                               const float* scale, const float* shift, const float* coef, int N, int H,
                               int W, int C, int sh, int inner_relu, int accumulate, hr_stream_t stream) {
  OP_BEGIN(HR_OP_GRAD_TERM);
  op.i[HR_GRAD_TERM_I_DTYPE] = dtype; op.i[HR_GRAD_TERM_I_N] = N; op.i[HR_GRAD_TERM_I_H] = H;
  op.i[HR_GRAD_TERM_I_W] = W; op.i[HR_GRAD_TERM_I_C] = C; op.i[HR_GRAD_TERM_I_SH] = sh;
  op.i[HR_GRAD_TERM_I_INNER_RELU] = inner_relu; op.i[HR_GRAD_TERM_I_ACCUMULATE] = accumulate;
  op.p[HR_GRAD_TERM_P_DST] = dst; op.p[HR_GRAD_TERM_P_G] = (void*)g; op.p[HR_GRAD_TERM_P_MASK] = (void*)mask_out;
  op.p[HR_GRAD_TERM_P_Y] = (void*)y;
  op.p[HR_GRAD_TERM_P_SCALE] = (void*)scale; op.p[HR_GRAD_TERM_P_SHIFT] = (void*)shift;
  op.p[HR_GRAD_TERM_P_COEF] = (void*)coef;
  return hr_launch_grad_term(op, (hipStream_t)stream);
}

extern "C" int hrnet_grad_term2(int dtype, void* dst, void* dst2, const void* g, const void* mask_out,
                                const void* y, const float* scale, const float* shift, const float* coef, int N,
                                int H, int W, int C, int accumulate, int accumulate2, hr_stream_t stream) {
  OP_BEGIN(HR_OP_GRAD_TERM);
  op.i[HR_GRAD_TERM_I_DTYPE] = dtype; op.i[HR_GRAD_TERM_I_N] = N; op.i[HR_GRAD_TERM_I_H] = H;
  op.i[HR_GRAD_TERM_I_W] = W; op.i[HR_GRAD_TERM_I_C] = C; op.i[HR_GRAD_TERM_I_ACCUMULATE] = accumulate;
  op.i[HR_GRAD_TERM_I_ACCUMULATE2] = accumulate2;
  op.p[HR_GRAD_TERM_P_DST] = dst; op.p[HR_GRAD_TERM_P_G] = (void*)g; op.p[HR_GRAD_TERM_P_MASK] = (void*)mask_out;
  op.p[HR_GRAD_TERM_P_Y] = (void*)y;
  op.p[HR_GRAD_TERM_P_SCALE] = (void*)scale; op.p[HR_GRAD_TERM_P_SHIFT] = (void*)shift;
  op.p[HR_GRAD_TERM_P_COEF] = (void*)coef; op.p[HR_GRAD_TERM_P_DST2] = dst2;
  return hr_launch_grad_term(op, (hipStream_t)stream);
}

extern "C" int hrnet_bn_bwd_reduce(int dtype, float* partials, const void* g, const void* mask_out,
                                   const void* y, const float* scale, const float* shift, int N, int H,
                                   int W, int C, int sh, int inner_relu, hr_stream_t stream) {
  OP_BEGIN(HR_OP_BN_BWD_REDUCE);
  op.i[HR_BN_BWD_REDUCE_I_DTYPE] = dtype; op.i[HR_BN_BWD_REDUCE_I_N] = N; op.i[HR_BN_BWD_REDUCE_I_H] = H;
  op.i[HR_BN_BWD_REDUCE_I_W] = W; op.i[HR_BN_BWD_REDUCE_I_C] = C; op.i[HR_BN_BWD_REDUCE_I_SH] = sh;
  op.i[HR_BN_BWD_REDUCE_I_INNER_RELU] = inner_relu;
  op.p[HR_BN_BWD_REDUCE_P_PARTIALS] = partials; op.p[HR_BN_BWD_REDUCE_P_G] = (void*)g;
  op.p[HR_BN_BWD_REDUCE_P_MASK] = (void*)mask_out; op.p[HR_BN_BWD_REDUCE_P_Y] = (void*)y;
  op.p[HR_BN_BWD_REDUCE_P_SCALE] = (void*)scale; op.p[HR_BN_BWD_REDUCE_P_SHIFT] = (void*)shift;
  return hr_launch_bn_bwd_reduce(op, (hipStream_t)stream);
}

extern "C" int hrnet_bn_bwd_finalize(const float* partials, int blocks, int C, float count,
                                     const float* gamma, const float* save_mean, const float* save_invstd,
                                     float* dgamma, float* dbeta, float* coef, int accumulate,
                                     hr_stream_t stream) {
  OP_BEGIN(HR_OP_BN_BWD_FINALIZE);
  op.i[HR_BN_BWD_FINALIZE_I_BLOCKS] = blocks; op.i[HR_BN_BWD_FINALIZE_I_C] = C;
  op.i[HR_BN_BWD_FINALIZE_I_ACCUMULATE] = accumulate;
  op.f[HR_BN_BWD_FINALIZE_F_COUNT] = count;
  op.p[HR_BN_BWD_FINALIZE_P_PARTIALS] = (void*)partials; op.p[HR_BN_BWD_FINALIZE_P_GAMMA] = (void*)gamma;
  op.p[HR_BN_BWD_FINALIZE_P_SAVE_MEAN] = (void*)save_mean;
  op.p[HR_BN_BWD_FINALIZE_P_SAVE_INVSTD] = (void*)save_invstd; op.p[HR_BN_BWD_FINALIZE_P_DGAMMA] = dgamma;
  op.p[HR_BN_BWD_FINALIZE_P_DBETA] = dbeta; op.p[HR_BN_BWD_FINALIZE_P_COEF] = coef;
  return hr_launch_bn_bwd_finalize(op, (hipStream_t)stream);
}

static void fill_cat(HrOp& op, int dtype, const int* hs, const int* ws, const int* cs, int nbr, int N,
                     int H, int W) {
  op.i[HR_CAT_I_DTYPE] = dtype; op.i[HR_CAT_I_NBR] = nbr; op.i[HR_CAT_I_N] = N; op.i[HR_CAT_I_H] = H;
  op.i[HR_CAT_I_W] = W;
  for (int k = 0; k < nbr && k < 4; ++k) {
    op.i[HR_CAT_I_HS0 + k] = hs[k]; op.i[HR_CAT_I_WS0 + k] = ws[k]; op.i[HR_CAT_I_CS0 + k] = cs[k];
  }
}

extern "C" int hrnet_bilinear_cat(int dtype, void* cat, const void* const* xs, const int* hs,
                                  const int* ws, const int* cs, int nbr, int N, int H, int W,
                                  int align_corners, hr_stream_t stream) {
  OP_BEGIN(HR_OP_BILINEAR_CAT);
  HR_REQUIRE(nbr >= 1 && nbr <= 4 && xs && hs && ws && cs, "bilinear_cat: args");
  fill_cat(op, dtype, hs, ws, cs, nbr, N, H, W);
  op.f[HR_CAT_F_ALIGN] = align_corners ? 1.f : 0.f;
  op.p[HR_CAT_P_CAT] = cat;
  for (int k = 0; k < nbr; ++k) op.p[HR_CAT_P_X0 + k] = (void*)xs[k];
  return hr_launch_bilinear_cat(op, (hipStream_t)stream);
}

extern "C" int hrnet_bilinear_cat_bwd(int dtype, const void* dcat, void* const* dxs, const int* hs,
                                      const int* ws, const int* cs, int nbr, int N, int H, int W,
                                      int align_corners, int accumulate, hr_stream_t stream) {
  OP_BEGIN(HR_OP_BILINEAR_CAT_BWD);
  HR_REQUIRE(nbr >= 1 && nbr <= 4 && dxs && hs && ws && cs, "bilinear_cat_bwd: args");
  fill_cat(op, dtype, hs, ws, cs, nbr, N, H, W);
  op.f[HR_CAT_F_ALIGN] = align_corners ? 1.f : 0.f;
  op.i[HR_CAT_I_ACCUMULATE] = accumulate;
  op.p[HR_CAT_P_CAT] = (void*)dcat;
  for (int k = 0; k < nbr; ++k) op.p[HR_CAT_P_X0 + k] = dxs[k];
  return hr_launch_bilinear_cat_bwd(op, (hipStream_t)stream);
}

extern "C" int hrnet_head_mix(int dtype, const void* x0, const void* w0, const float* bias, void* y, float* stats,
                              int rows_mode, const void* const* ts, const int* hs, const int* ws, int nup, int N, int H,
                              int W, int C0, int Cout, int align_corners, hr_stream_t stream) {
  OP_BEGIN(HR_OP_HEAD_MIX);
  HR_REQUIRE(nup >= 0 && nup <= 3 && (nup == 0 || (ts && hs && ws)), "head_mix: args");
  op.i[HR_HEAD_MIX_I_DTYPE] = dtype; op.i[HR_HEAD_MIX_I_N] = N; op.i[HR_HEAD_MIX_I_H] = H;
  op.i[HR_HEAD_MIX_I_W] = W; op.i[HR_HEAD_MIX_I_C0] = C0; op.i[HR_HEAD_MIX_I_COUT] = Cout;
  op.i[HR_HEAD_MIX_I_NUP] = nup; op.i[HR_HEAD_MIX_I_ALIGN] = align_corners;
  op.i[HR_HEAD_MIX_I_ROWS_MODE] = rows_mode;
  op.p[HR_HEAD_MIX_P_X0] = (void*)x0; op.p[HR_HEAD_MIX_P_W0] = (void*)w0; op.p[HR_HEAD_MIX_P_BIAS] = (void*)bias;
  op.p[HR_HEAD_MIX_P_Y] = y; op.p[HR_HEAD_MIX_P_STATS] = stats;
  for (int k = 0; k < nup; ++k) {
    op.i[HR_HEAD_MIX_I_UP_H1 + 2 * k] = hs[k]; op.i[HR_HEAD_MIX_I_UP_W1 + 2 * k] = ws[k];
    op.p[HR_HEAD_MIX_P_T1 + k] = (void*)ts[k];
  }
  return hr_launch_head_mix(op, (hipStream_t)stream);
}

extern "C" int hrnet_upsample_bilinear_t(int dtype, const void* g, void* const* outs, const int* hs, const int* ws,
                                         int nout, int N, int H, int W, int C, int align_corners, int streamed,
                                         hr_stream_t stream) {
  OP_BEGIN(HR_OP_UPSAMPLE_T);
  HR_REQUIRE(nout >= 1 && nout <= 3 && outs && hs && ws, "upsample_t: args");
  op.i[HR_UPSAMPLE_T_I_DTYPE] = dtype; op.i[HR_UPSAMPLE_T_I_N] = N; op.i[HR_UPSAMPLE_T_I_H] = H;
  op.i[HR_UPSAMPLE_T_I_W] = W; op.i[HR_UPSAMPLE_T_I_C] = C; op.i[HR_UPSAMPLE_T_I_NOUT] = nout;
  op.i[HR_UPSAMPLE_T_I_ALIGN] = align_corners;
  op.i[HR_UPSAMPLE_T_I_STREAMED] = streamed;
  op.p[HR_UPSAMPLE_T_P_G] = (void*)g;
  for (int k = 0; k < nout; ++k) {
    op.p[HR_UPSAMPLE_T_P_OUT1 + k] = outs[k];
    op.i[HR_UPSAMPLE_T_I_OUT_H1 + 2 * k] = hs[k]; op.i[HR_UPSAMPLE_T_I_OUT_W1 + 2 * k] = ws[k];
  }
  return hr_launch_upsample_t(op, (hipStream_t)stream);
}

extern "C" int hrnet_head_bwd(int dtype, int mode, const void* dy, const void* wT, const void* y, void* out,
                              const float* bn_scale, const float* bn_shift, const float* coef, int inner_relu, int N,
                              int H, int W, int K, int Cout, hr_stream_t stream) {
  OP_BEGIN(HR_OP_HEAD_BWD);
  op.i[HR_HEAD_BWD_I_DTYPE] = dtype; op.i[HR_HEAD_BWD_I_N] = N; op.i[HR_HEAD_BWD_I_H] = H;
  op.i[HR_HEAD_BWD_I_W] = W; op.i[HR_HEAD_BWD_I_K] = K; op.i[HR_HEAD_BWD_I_COUT] = Cout;
  op.i[HR_HEAD_BWD_I_MODE] = mode; op.i[HR_HEAD_BWD_I_INNER_RELU] = inner_relu;
  op.p[HR_HEAD_BWD_P_DY] = (void*)dy; op.p[HR_HEAD_BWD_P_WT] = (void*)wT; op.p[HR_HEAD_BWD_P_Y] = (void*)y;
  op.p[HR_HEAD_BWD_P_OUT] = out;
  op.p[HR_HEAD_BWD_P_BN_SCALE] = (void*)bn_scale; op.p[HR_HEAD_BWD_P_BN_SHIFT] = (void*)bn_shift;
  op.p[HR_HEAD_BWD_P_COEF] = (void*)coef;
  return hr_launch_head_bwd(op, (hipStream_t)stream);
}

extern "C" int hrnet_im2col_stem(int dtype, const float* img_nchw, void* cols, int N, int C, int H, int W,
                                 int Ho, int Wo, int Kpad, hr_stream_t stream) {
  OP_BEGIN(HR_OP_IM2COL_STEM);
  op.i[HR_IM2COL_I_DTYPE] = dtype; op.i[HR_IM2COL_I_N] = N; op.i[HR_IM2COL_I_C] = C; op.i[HR_IM2COL_I_H] = H;
  op.i[HR_IM2COL_I_W] = W; op.i[HR_IM2COL_I_HO] = Ho; op.i[HR_IM2COL_I_WO] = Wo; op.i[HR_IM2COL_I_KPAD] = Kpad;
  op.p[HR_IM2COL_P_IMG] = (void*)img_nchw; op.p[HR_IM2COL_P_COLS] = cols;
  return hr_launch_im2col_stem(op, (hipStream_t)stream);
}

extern "C" int hrnet_nhwc_to_nchw(int dtype, const void* src, float* dst, int N, int H, int W, int Cp,
                                  int C, hr_stream_t stream) {
  OP_BEGIN(HR_OP_NHWC_TO_NCHW);
  op.i[HR_LAYOUT_I_DTYPE] = dtype; op.i[HR_LAYOUT_I_N] = N; op.i[HR_LAYOUT_I_H] = H; op.i[HR_LAYOUT_I_W] = W;
  op.i[HR_LAYOUT_I_CP] = Cp; op.i[HR_LAYOUT_I_C] = C;
  op.p[HR_LAYOUT_P_SRC] = (void*)src; op.p[HR_LAYOUT_P_DST] = dst;
  return hr_launch_nhwc_to_nchw(op, (hipStream_t)stream);
}

extern "C" int hrnet_nchw_to_nhwc(int dtype, const float* src, void* dst, int N, int H, int W, int Cp,
                                  int C, hr_stream_t stream) {
  OP_BEGIN(HR_OP_NCHW_TO_NHWC);
  op.i[HR_LAYOUT_I_DTYPE] = dtype; op.i[HR_LAYOUT_I_N] = N; op.i[HR_LAYOUT_I_H] = H; op.i[HR_LAYOUT_I_W] = W;
  op.i[HR_LAYOUT_I_CP] = Cp; op.i[HR_LAYOUT_I_C] = C;
  op.p[HR_LAYOUT_P_SRC] = (void*)src; op.p[HR_LAYOUT_P_DST] = dst;
  return hr_launch_nchw_to_nhwc(op, (hipStream_t)stream);
}

extern "C" int hrnet_bias_grad(int dtype, const void* dy, float* dbias, float* scratch, int pixels, int Cp,
                               int C, int accumulate, hr_stream_t stream) {
  OP_BEGIN(HR_OP_BIAS_GRAD);
  op.i[HR_BIAS_GRAD_I_DTYPE] = dtype; op.i[HR_BIAS_GRAD_I_PIXELS] = pixels; op.i[HR_BIAS_GRAD_I_CP] = Cp;
  op.i[HR_BIAS_GRAD_I_C] = C; op.i[HR_BIAS_GRAD_I_ACCUMULATE] = accumulate;
  op.p[HR_BIAS_GRAD_P_DY] = (void*)dy; op.p[HR_BIAS_GRAD_P_DBIAS] = dbias; op.p[HR_BIAS_GRAD_P_SCRATCH] = scratch;
  return hr_launch_bias_grad(op, (hipStream_t)stream);
}

extern "C" int hrnet_fill_zero(void* p, int64_t bytes, hr_stream_t stream) {
  OP_BEGIN(HR_OP_FILL);
  op.i[HR_FILL_I_BYTES_LO] = (int32_t)(uint32_t)(bytes & 0xffffffffLL);
  op.i[HR_FILL_I_BYTES_HI] = (int32_t)(uint32_t)((uint64_t)bytes >> 32);
  op.p[HR_FILL_P_DST] = p;
  return hr_launch_fill(op, (hipStream_t)stream);
}
